"""GPU: U-IDS / P-IDS on the device (sh-gan_amd/ids_score.py, csrc/svm.hip) -- the streaming pass in both modes against numpy float64 on
the same float32 rows, the fit at the five cases of tests/ids_f64.py against that yardstick's optimum, the kernels a fit launches, EvalLoop's
``pids_uids`` option, and the fill / guard runs of the new allocation sites (they are newer than the site tables of
tests/test_gpu_alloc_fill.py / test_gpu_alloc_guard.py)."""
import numpy as np
import pytest
import torch

import ids_f64 as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-9

# (n0, n1, D): every N of {1, 2, 63, 64, 65, 130} and every D of {1, 3, 255, 256, 257, 2048, 4096}; unequal sets, one set only (n1 = 0);
# D = 252 / 2044: 16-byte loads whose last one of a row would start past column D.  In all of these a wave has at most one row (the grid is
# min(cap, ceil(n / 4)) workgroups of four waves, cap = 512 up to D = 2048 and 256 above).
PASS_CASES = [(1, 1, 1), (2, 1, 3), (63, 65, 255), (64, 64, 256), (65, 2, 257), (130, 63, 2048), (64, 130, 4096), (130, 0, 256), (1, 0, 2048),
              (2, 0, 3), (65, 63, 252), (5, 3, 2044), (520, 517, 24), (63, 0, 4096), (3, 2, 1300)]
# n > 4 cap: the steady-state loop -- the next row's prefetch, its hand-over and the accumulation over several rows of one wave.  5100 rows of
# 2048 (8 chunks, 16-byte loads) and of 2047 (dword loads) on 2048 waves: two rows per wave, three for the first 1004; 2500 rows of 4096
# (16 chunks; the cap of 256 workgroups binds: two rows per wave, three for the first 452); 4300 rows of 24 (one chunk: two rows, three
# for the first 204); 2500 rows of one set at 500 columns (2 chunks, the last one ragged: the first 452 waves get two rows)
MULTI_ROUND_CASES = [(2600, 2500, 2048), (1300, 1200, 4096), (2600, 2500, 2047), (2200, 2100, 24), (2500, 0, 500)]
PASS_CASES += MULTI_ROUND_CASES


def _operands(n0, n1, D, seed):
    """Rows like pooled activations (non-negative, unequal norms) and a v that leaves rows on both sides of the hinge."""
    g = np.random.RandomState(seed)
    rows = lambda n: (np.abs(g.standard_normal((n, D))) * 0.5 * (0.5 + g.rand(n, 1))).astype(np.float32)        # noqa: E731
    x0, x1 = rows(n0), (rows(n1) if n1 else None)
    v = g.standard_normal(D + 1) * 1.5 / np.sqrt(D)
    v[D] = 0.3
    return x0, x1, v


def _dev(x):
    return None if x is None else torch.from_numpy(x).to(DEV)


@pytest.mark.parametrize('n0,n1,D', PASS_CASES)
def test_pass_against_float64_in_both_modes(n0, n1, D):
    from shgan_amd import ids_score
    x0, x1, v = _operands(n0, n1, D, seed=n0 * 7 + n1 * 3 + D)
    n, C = n0 + n1, 0.75
    q_ref, z_ref, a_ref, bq, bz = ref.pass_f64(x0, x1, v, 'grad', C)
    y = np.concatenate([np.ones(n0), -np.ones(n1)])
    margin = np.abs(1.0 - y * z_ref)
    assert np.all(margin > bz), 'a case must have no row inside the rounding band of the hinge (the reference alone decides this)'
    assert n < 16 or 0 < a_ref.sum() < n                                  # rows on both sides of the hinge
    d0, d1, dv = _dev(x0), _dev(x1), torch.from_numpy(v).to(DEV)
    q, z, a = ids_score.svm_pass(d0, d1, dv, 'grad', C=C)
    q2, z2, a2 = ids_score.svm_pass(d0, d1, dv, 'grad', C=C)
    assert q.shape == (D + 2,) and z.shape == (n,) and a.shape == (n,) and a.dtype == torch.uint8 and q.dtype == z.dtype == torch.float64
    assert torch.equal(q, q2) and torch.equal(z, z2) and torch.equal(a, a2)                                     # the same bits on every run
    q, z, a = q.cpu().numpy(), z.cpu().numpy(), a.cpu().numpy()
    print(f'grad ({n0}, {n1}, {D}): max |z - ref| / bound {np.max(np.abs(z - z_ref) / bz):.3e}, max |q - ref| / bound '
          f'{np.max(np.abs(q[:D + 1] - q_ref[:D + 1]) / np.maximum(bq, 1e-300)):.3e}, active {int(a_ref.sum())} of {n}')
    assert np.all(np.abs(z - z_ref) <= bz)
    assert np.array_equal(a, a_ref)
    assert np.all(np.abs(q[:D + 1] - q_ref[:D + 1]) <= bq)
    # the loss: each active term (1 - y z)^2 moves by at most 2 |m| bz + bz^2 (plus its own rounding), the sum by gamma_n
    m = margin * a_ref
    gam = (n + 4) * 2.0 ** -53
    assert abs(q[D + 1] - q_ref[D + 1]) <= float((a_ref * (2 * m * bz + bz * bz)).sum() + gam * (m * m).sum())
    # hv: the active set is an operand (here: the grad pass's, with every third row flipped), v another vector
    act = a_ref.copy()
    act[::3] ^= 1
    u = np.random.RandomState(D + n).standard_normal(D + 1)
    q_ref, z_ref, _, bq, bz = ref.pass_f64(x0, x1, u, 'hv', C, a=act)
    du, da = torch.from_numpy(u).to(DEV), torch.from_numpy(act).to(DEV)
    q, z, a_back = ids_score.svm_pass(d0, d1, du, 'hv', C=C, a=da)
    q2, z2, _ = ids_score.svm_pass(d0, d1, du, 'hv', C=C, a=da)
    assert torch.equal(q, q2) and torch.equal(z, z2) and torch.equal(a_back, da)
    q, z = q.cpu().numpy(), z.cpu().numpy()
    print(f'hv   ({n0}, {n1}, {D}): max |z - ref| / bound {np.max(np.abs(z - z_ref) / bz):.3e}, max |q - ref| / bound '
          f'{np.max(np.abs(q[:D + 1] - q_ref[:D + 1]) / np.maximum(bq, 1e-300)):.3e}')
    assert np.all(np.abs(z - z_ref) <= bz) and np.all(np.abs(q[:D + 1] - q_ref[:D + 1]) <= bq) and q[D + 1] == 0.0


@pytest.mark.parametrize('D,pitch,offset', [(256, 260, 0), (252, 256, 0), (255, 300, 0), (2044, 2048, 4), (24, 25, 1), (4096, 4100, 0)])
def test_row_pitch_views_are_served_and_never_read_past_the_row(D, pitch, offset):
    """svm_pass documents that a view with a row pitch larger than D is served without a copy.  The columns beside the rows hold NaN: one
    load past column D (or in front of column 0) would reach q or z.  Same bits as the contiguous copy: the lanes' columns are the same
    whether the loads are 16-byte or dword."""
    from shgan_amd import ids_score
    n0, n1 = 9, 6
    x0, x1, v = _operands(n0, n1, D, seed=D + pitch)
    big0 = torch.full((n0, pitch), float('nan'), device=DEV)
    big1 = torch.full((n1, pitch), float('nan'), device=DEV)
    v0, v1 = big0[:, offset:offset + D], big1[:, offset:offset + D]
    v0.copy_(torch.from_numpy(x0))
    v1.copy_(torch.from_numpy(x1))
    assert not v0.is_contiguous() and v0.stride(0) == pitch
    dv = torch.from_numpy(v).to(DEV)
    q, z, a = ids_score.svm_pass(v0, v1, dv, 'grad')
    qc, zc, ac = ids_score.svm_pass(_dev(x0), _dev(x1), dv, 'grad')
    assert torch.equal(q, qc) and torch.equal(z, zc) and torch.equal(a, ac) and bool(torch.isfinite(q).all())
    q_ref, z_ref, a_ref, bq, bz = ref.pass_f64(x0, x1, v, 'grad')
    assert np.all(np.abs(z.cpu().numpy() - z_ref) <= bz) and np.all(np.abs(q.cpu().numpy()[:D + 1] - q_ref[:D + 1]) <= bq)
    qh, zh, _ = ids_score.svm_pass(v0, v1, dv, 'hv', a=a)
    qhc, zhc, _ = ids_score.svm_pass(_dev(x0), _dev(x1), dv, 'hv', a=a)
    assert torch.equal(qh, qhc) and torch.equal(zh, zhc) and bool(torch.isfinite(qh).all())
    assert bool(torch.isnan(big0[:, offset + D:]).all()) and bool(torch.isnan(big0[:, :offset]).all())         # and nothing was written there


def test_wrapper_refuses_what_it_does_not_serve():
    from shgan_amd import _lib, ids_score
    x = torch.zeros(8, 16, device=DEV)
    v = torch.zeros(17, dtype=torch.float64, device=DEV)
    for args, kw in (((x.t(), None, v, 'grad'), {}), ((x, x[:, :8], v, 'grad'), {}), ((x, None, v[:16], 'grad'), {}), ((x, None, v.float(), 'grad'), {}),
                     ((x, None, v, 'hv'), {}), ((x, None, v, 'hv'), dict(a=torch.zeros(7, dtype=torch.uint8, device=DEV))),
                     ((x, None, v, 'grad'), dict(a=torch.zeros(8, dtype=torch.uint8, device=DEV))), ((x.double(), None, v, 'grad'), {}),
                     ((torch.zeros(2, 4097, device=DEV), None, torch.zeros(4098, dtype=torch.float64, device=DEV), 'grad'), {})):
        with pytest.raises(_lib.ShgError):
            ids_score.svm_pass(*args, **kw)
    with pytest.raises(_lib.ShgError):
        ids_score.ids_from_features(x, x[:4])
    with pytest.raises(_lib.ShgError):
        ids_score.ids_from_features(x[:, :8], x[:, :8])


_YARD = {}


def _yardstick(case):
    if case not in _YARD:
        real, fake = ref.features(*ref.CASES[case])
        _YARD[case] = (real, fake) + ref.fit(real, fake)
    return _YARD[case]


@pytest.mark.parametrize('case', list(ref.CASES))
def test_fit_reaches_the_optimum_and_the_yardsticks_counts(case):
    """|grad f| at the returned (w, b), recomputed in numpy float64, meets the stopping rule; by 1-strong convexity |v - v*| <= |grad f(v)|
    for both solutions, so every decision is within |x~_i| (|grad f_dev| + |grad f_ref|) + gamma_(D+2) sum |x~_i| |w| of the yardstick's.
    Precondition (on the yardstick alone, with the largest |grad f_dev| the stopping rule admits): every |dec| and every |dec(fake_i) -
    dec(real_i)| is at least 10 x that bound.  Then no sample may be counted differently: the integer counts are equal."""
    from shgan_amd import ids_score
    real, fake, v_ref, info = _yardstick(case)
    N, D = real.shape
    Xt, y = ref.stack(real, fake)
    g0 = info['grad_norm0']
    rows, gam = np.linalg.norm(Xt, axis=1), (D + 2) * 2.0 ** -53 / (1 - (D + 2) * 2.0 ** -53)
    dr, df = ref.decisions(v_ref, real, fake)
    worst = rows * (TOL * g0 * (1 + 1e-6) + info['grad_norm']) + gam * (np.abs(Xt) @ np.abs(v_ref))
    assert np.all(np.abs(np.concatenate([dr, df])) >= 10 * worst) and np.all(np.abs(df - dr) >= 10 * (worst[:N] + worst[N:]))
    res = ids_score.ids_from_features(torch.from_numpy(real).to(DEV), torch.from_numpy(fake).to(DEV), tol=TOL)
    v = np.concatenate([res['w'].cpu().numpy(), [res['b']]])
    g = float(np.linalg.norm(ref.gradient(v, Xt, y)))
    print(f"case {case}: {res['newton_iters']} Newton steps, {res['passes']} passes, |grad| / |grad(0)| = {g / g0:.3e} (device: "
          f"{res['grad_norm'] / res['grad_norm0']:.3e}), |v - v_ref| = {np.linalg.norm(v - v_ref):.3e}")
    assert res['converged'] and abs(res['grad_norm0'] - g0) <= 1e-12 * g0
    assert g <= TOL * g0 * (1 + 1e-6)
    bound = rows * (g + info['grad_norm']) + gam * (np.abs(Xt) @ np.abs(v))
    dec = res['dec'].cpu().numpy()
    assert dec.shape == (2 * N,) and np.all(np.abs(dec - np.concatenate([dr, df])) <= bound)
    assert (res['uids_errors'], res['pids_wins']) == ref.ids(v_ref, real, fake)[2:]
    assert (res['uids'], res['pids']) == ref.ids(v_ref, real, fake)[:2] and res['n'] == N
    assert (round(res['uids'], 4), round(res['pids'], 4)) == ref.SCORES[case]


def test_fit_runs_the_pass_kernel_and_no_blas_gemm():
    import route_probe
    from shgan_amd import ids_score
    real, fake = (torch.from_numpy(t).to(DEV) for t in ref.features(*ref.CASES['B']))
    fit, names = route_probe.launched(lambda: ids_score.fit_linear_svc(real, fake), expect=('svm_pass_kernel', 'svm_reduce_kernel'))
    assert fit['converged']
    assert route_probe.any_hit('svm_pass_kernel', names) and route_probe.any_hit('svm_reduce_kernel', names), sorted(names)
    assert not [n for n in names if 'Cijk_' in n], sorted(names)


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


def test_eval_loop_pids_uids(small_g):
    """96 items, batch 16, two streams, a stand-in detector of width 32: ids_value() equals ids_from_features on the features of the
    gathered images and the loader's reals; with kid beside it there is one pair of row buffers; off, images and moments are the same bits."""
    from shgan_amd import eval_harness as hz, ids_score, kernels
    n_items, b, R, W = 96, 16, 256, 32

    def feats(img, input_range='0_255'):
        if input_range == 'pm1':
            img = (kernels.u8_value_table(DEV)[img.long()] if img.dtype == torch.uint8 else img) * 127.5 + 127.5
        return hz.standin_features(img, W) / 64

    def run(**kw):
        loop = hz.EvalLoop(small_g, DEV, R, n_items, noise_mode='const', depth=2, latent_fn=_latents, feature_fn=feats, fid_dim=W, fid_real=True, **kw)
        np.random.seed(21)
        loop.run(hz.PinnedU8Loader(loop.ids, b, R, seed=13))
        return loop, loop.gather()
    loop, (images, fid) = run(pids_uids=True)
    both, _ = run(pids_uids=dict(tol=1e-9), kid=dict(num_subsets=2, max_subset_size=16, seed=1))
    plain, (images0, fid0) = run()
    torch.cuda.synchronize()
    assert plain.kid_features is None and plain.evaluators['detector'].ids_opts is None and plain.evaluators['detector'].kid_local is None
    with pytest.raises(ValueError):
        plain.ids_value()
    with pytest.raises(ValueError):
        loop.kid_value()
    assert torch.equal(images, images0) and torch.equal(fid.S, fid0.S) and torch.equal(loop.fid_real.S, plain.fid_real.S)
    reals = torch.cat([img for img, _ in hz.PinnedU8Loader(list(range(n_items)), b, R, seed=13)]).to(DEV)
    f_fake = torch.cat([feats(images[k:k + b]) for k in range(0, n_items, b)])
    f_real = torch.cat([feats(reals[k:k + b], input_range='pm1') for k in range(0, n_items, b)])
    fake, real = loop.kid_features
    assert fake.shape == (n_items, W) and torch.equal(fake, f_fake) and torch.equal(real, f_real)
    assert all(torch.equal(s, t) for s, t in zip(both.kid_features, loop.kid_features))
    want = ids_score.ids_from_features(f_real.contiguous(), f_fake.contiguous())
    got = loop.ids_value()
    print(f"loop U-IDS {got[0]:.6f}, P-IDS {got[1]:.6f} ({want['newton_iters']} Newton steps, {want['passes']} passes)")
    assert got == (want['uids'], want['pids']) == both.ids_value()
    assert both.evaluators['detector'].kid_opts is not None and loop.evaluators['detector'].kid_opts is None


# (N, D): the last 16-byte load of a row would start at column D (252: lanes 63; 2044: chunk 7's lane 63) and, in the last row, past the
# buffer; 255 / 3: dword loads, D + 1 would be the next row or the end
GUARD_CASES = [(5, 252), (3, 2044), (6, 255), (9, 3)]


@pytest.mark.parametrize('N,D', GUARD_CASES)
def test_pass_and_fit_do_not_depend_on_fresh_contents_and_stay_inside_their_buffers(N, D):
    """('ids_score.py', 'svm_pass') and ('ids_score.py', 'fit_linear_svc'): the same bits with every fresh allocation pre-filled with NaN
    bytes and with large values, and no guard band touched with every buffer, the feature rows, v and a included, housed between poisoned
    bands."""
    import alloc_fill
    import alloc_guard
    from shgan_amd import ids_score
    real, fake = ref.features(N, D, 0.2, seed=D)
    v = np.random.RandomState(N).standard_normal(D + 1) / np.sqrt(D)

    def run():
        r, f, dv = torch.from_numpy(real).to(DEV), torch.from_numpy(fake).to(DEV), torch.from_numpy(v).to(DEV)
        q, z, a = ids_score.svm_pass(r, f, dv, 'grad')
        qh, zh, _ = ids_score.svm_pass(r, None, dv, 'hv', a=a[:N].contiguous())
        res = ids_score.ids_from_features(r, f)
        return [q, z, a, qh, zh, res['w'], res['dec']], (res['b'], res['uids_errors'], res['pids_wins'], res['passes'])
    want, want_s = run()
    torch.cuda.synchronize()
    for pattern in ('nan', 'big'):
        with alloc_fill.filled(pattern) as rec:
            got, got_s = run()
            torch.cuda.synchronize()
        assert {('ids_score.py', 'svm_pass'), ('ids_score.py', 'fit_linear_svc')} <= rec.sites, rec.sites
        assert got_s == want_s and all(torch.equal(g, w) for g, w in zip(got, want)), pattern
    with alloc_guard.guarded() as rec:
        got, got_s = run()
        bad = rec.violations()
        assert {('ids_score.py', 'svm_pass'), ('ids_score.py', 'fit_linear_svc')} <= rec.sites and not bad, bad
        assert got_s == want_s and all(torch.equal(g, w) for g, w in zip(got, want))
