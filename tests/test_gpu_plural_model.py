"""GPU: K completions per masked input through the module API -- ``Generator.encode`` / ``synthesize`` / ``sample_many`` and
``Synthesis_Plur`` -- at the reduced 256 generator of tests/golden/generator_small.npz (ch_base 2048, ch_max 32, w_dim 64, z_dim 64, w0_dim
128; its weights and its N = 2 masked inputs), K = 3.  On the commit before this feature every test fails with a missing attribute
(``Generator.encode``, ``sample_many``), registry name or ``model_cfg`` argument."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K = 3
KW = dict(ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128)


def c(a):
    return a.detach().cpu().numpy()


@pytest.fixture(scope='module')
def env():
    """The generator_small weights in three generators (plain, Synthesis_Plur, fp16 blocks) and the fixture's inputs; z [2,3,64] with
    z[:, 0] the fixture's own."""
    import shgan_amd  # noqa: F401
    from shgan_amd import configs, eval_harness
    from oracle import shgan_oracle as orc
    g = load_golden('generator_small')
    sd = orc.init_state_dict(256, seed=int(g['seed']), noise_strength=0.1, bias_std=0.1, **KW)

    def make(**kw):
        G = configs.build_generator(256, **KW, **kw)
        G.load_state_dict(sd, strict=True)
        return G.eval().requires_grad_(False).to(DEV)
    real = torch.from_numpy(g['real_u8'].astype(np.float32)) / 127.5 - 1.0
    mask = torch.from_numpy(np.unpackbits(g['mask_bits'])[: 2 * 256 * 256].reshape(2, 1, 256, 256).astype(np.float32))
    x = eval_harness.assemble_input(real, mask).to(DEV)
    z0 = torch.from_numpy(g['z'])
    z = torch.cat([z0[:, None], torch.randn(2, K - 1, 64, generator=torch.Generator().manual_seed(31))], dim=1).to(DEV)
    return dict(make=make, G=make(), x=x, z=z, cnd=torch.zeros(2, 0, device=DEV), cnd_k=torch.zeros(2 * K, 0, device=DEV))


@pytest.fixture(scope='module')
def repeated(env):
    """The yardstick, computed once: the plain forward on the K-fold repeated input."""
    return env['G'](x=env['x'].repeat_interleave(K, 0), z=env['z'].flatten(0, 1), c=env['cnd_k'], noise_mode='const')


def test_forward_is_synthesize_of_encode(env):
    G, x, z, cnd = env['G'], env['x'], env['z'][:, 0].contiguous(), env['cnd']
    whole = G(x=x, z=z, c=cnd, noise_mode='const')
    enc = G.encode(x)
    assert tuple(enc[0].shape) == (2, 128) and sorted(enc[1]) == [4, 8, 16, 32, 64, 128, 256]
    assert torch.equal(G.synthesize(enc, z, cnd, noise_mode='const'), whole)
    assert torch.equal(G.synthesize(enc, z, cnd, truncation_psi=0.7, noise_mode='const'), G(x=x, z=z, c=cnd, truncation_psi=0.7, noise_mode='const'))


def test_sample_many_against_the_repeated_forward(env, repeated):
    """rel_err < 1e-3, the bar test_generator_small_golden holds the generator to (the encoder's routes may differ between batch N and N*K)."""
    G, x, z = env['G'], env['x'], env['z']
    imgs = G.sample_many(x, z, noise_mode='const')
    assert tuple(imgs.shape) == (2, K, 3, 256, 256) and imgs.dtype == torch.float32
    e = rel_err(c(imgs.flatten(0, 1)), c(repeated))
    print(f'sample_many vs G(x.repeat_interleave(K), z): rel_err {e:.3e}')
    assert e < 1e-3
    for n in range(2):
        for k in range(K):
            assert rel_err(c(imgs[n, k]), c(repeated[n * K + k])) < 1e-3, (n, k)
    assert torch.equal(G.sample_many(x, z, env['cnd_k'], noise_mode='const'), imgs)              # an explicit empty label: the same call


def test_expansion_inside_the_model_is_repeat_interleave(env):
    """synthesize on an encoding expanded by hand with torch gives sample_many's bits."""
    G, x, z = env['G'], env['x'], env['z']
    xg, feats = G.encode(x)
    by_hand = (xg.repeat_interleave(K, 0), {r: f.repeat_interleave(K, 0) for r, f in feats.items()})
    want = G.synthesize(by_hand, z.flatten(0, 1), env['cnd_k'], noise_mode='const')
    assert torch.equal(G.sample_many(x, z, noise_mode='const').flatten(0, 1), want)
    ex, ef = G.expand_encoding((xg, feats), K)
    assert torch.equal(ex, by_hand[0]) and all(torch.equal(ef[r], by_hand[1][r]) for r in feats)
    one = G.sample_many(x, z[:, :1], noise_mode='const')                                          # K = 1: a plain copy of the encoding
    assert torch.equal(one[:, 0], G(x=x, z=z[:, 0].contiguous(), c=env['cnd'], noise_mode='const'))


def test_equal_z_gives_equal_samples_with_const_noise_and_different_ones_with_random(env):
    G, x = env['G'], env['x']
    z = env['z'][:, :1].expand(-1, K, -1).contiguous()
    a = G.sample_many(x, z, noise_mode='const')
    for k in range(1, K):
        assert torch.equal(a[:, k], a[:, 0]), k
    torch.manual_seed(3)
    r = G.sample_many(x, z, noise_mode='random')
    assert bool(torch.isfinite(r).all())
    for k in range(1, K):
        assert rel_err(c(r[:, k]), c(r[:, 0])) > 1e-4, k                                         # every row drew its own noise
    assert rel_err(c(r[:, 0]), c(a[:, 0])) > 1e-4


def test_sample_many_with_fp16_blocks(env):
    """use_fp16_before_res / use_fp16_after_res as in tests/test_gpu_fp16.py's generator case (encoder blocks 256, 128 and synthesis blocks 64,
    128, 256 in half): the skip features are expanded as half-precision channels-last tensors; against the repeated forward at that
    file's generator-level bound, 2e-2."""
    G = env['make'](use_fp16_before_res=64, use_fp16_after_res=32)
    x, z = env['x'], env['z']
    xg, feats = G.encode(x)
    assert feats[256].dtype == feats[128].dtype == torch.float16 and feats[64].dtype == torch.float32
    ex, ef = G.expand_encoding((xg, feats), K)
    for r, f in feats.items():
        assert ef[r].dtype == f.dtype and ef[r].stride()[1:] == f.stride()[1:] and torch.equal(ef[r], f.repeat_interleave(K, 0)), r
    imgs = G.sample_many(x, z, noise_mode='const')
    want = G(x=x.repeat_interleave(K, 0), z=z.flatten(0, 1), c=env['cnd_k'], noise_mode='const')
    e = rel_err(c(imgs.flatten(0, 1)), c(want))
    print(f'fp16 blocks: sample_many vs repeated forward rel_err {e:.3e}')
    assert imgs.dtype == torch.float32 and bool(torch.isfinite(imgs).all()) and e < 2e-2


def test_synthesis_plur_against_the_reference(env):
    """tests/golden/synthesis_plur.npz (tools/gen_golden_plur.py: the reference's Synthesis_Plur on the generator_small weights and inputs)
    with the recorded eps injected: rel_err < 1e-3 on the whole image of input 0 and, for input 1, on every second row and column and on 8192
    sampled positions (the file's size limit does not leave room for both whole images).  eps = 0 is
    Synthesis bit for bit; without injection two calls differ."""
    g = load_golden('synthesis_plur')
    Gp, G, x, cnd = env['make'](synthesis='comodgan_synthesis_plur'), env['G'], env['x'], env['cnd']
    z = env['z'][:, 0].contiguous()
    eps = torch.from_numpy(g['eps']).to(DEV)
    assert rel_err(c(Gp.mapping(z, cnd)), g['ws']) < 1e-5 and rel_err(c(Gp.encode(x)[0]), g['xg']) < 1e-4
    img = Gp(x=x, z=z, c=cnd, noise_mode='const', w0_noise=eps)
    e_0 = rel_err(c(img)[0], g['img0'])
    e_ds = rel_err(c(img)[1, :, ::2, ::2], g['img1_ds2'])
    e_s = rel_err(c(img)[1].reshape(-1)[g['sample_idx']], g['sample_val'])
    print(f'Synthesis_Plur vs reference: image 0 {e_0:.3e}; image 1 strided {e_ds:.3e}, samples {e_s:.3e}')
    assert e_0 < 1e-3 and e_ds < 1e-3 and e_s < 1e-3
    plain = G(x=x, z=z, c=cnd, noise_mode='const')
    assert rel_err(c(img), c(plain)) > 1e-3                                                      # the perturbation really acts
    assert torch.equal(Gp(x=x, z=z, c=cnd, noise_mode='const', w0_noise=torch.zeros_like(eps)), plain)
    torch.manual_seed(11)
    a, b = Gp(x=x, z=z, c=cnd, noise_mode='const'), Gp(x=x, z=z, c=cnd, noise_mode='const')
    assert not torch.equal(a, b) and bool(torch.isfinite(a).all())
    from shgan_amd import _lib
    with pytest.raises(_lib.ShgError, match='w0_noise'):
        Gp(x=x, z=z, c=cnd, noise_mode='const', w0_noise=eps[:1])
    with pytest.raises(TypeError):
        G(x=x, z=z, c=cnd, noise_mode='const', w0_noise=eps)                                     # Synthesis has no such argument


def test_synthesis_plur_under_sample_many(env):
    """Every one of the N*K rows gets its own draw: equal z and 'const' noise still give K different samples; zero draws give the plain
    generator's sample_many bit for bit, injected draws the rows of the repeated forward with the same draws."""
    Gp, G, x, z = env['make'](synthesis='comodgan_synthesis_plur'), env['G'], env['x'], env['z']
    same_z = z[:, :1].expand(-1, K, -1).contiguous()
    torch.manual_seed(12)
    s = Gp.sample_many(x, same_z, noise_mode='const')
    for k in range(1, K):
        assert rel_err(c(s[:, k]), c(s[:, 0])) > 1e-4, k
    zero = torch.zeros(2 * K, 128, device=DEV)
    assert torch.equal(Gp.sample_many(x, z, noise_mode='const', w0_noise=zero), G.sample_many(x, z, noise_mode='const'))
    eps = torch.randn(2 * K, 128, generator=torch.Generator().manual_seed(13)).to(DEV)
    got = Gp.sample_many(x, z, noise_mode='const', w0_noise=eps).flatten(0, 1)
    want = Gp(x=x.repeat_interleave(K, 0), z=z.flatten(0, 1), c=env['cnd_k'], noise_mode='const', w0_noise=eps)
    assert rel_err(c(got), c(want)) < 1e-3


def test_sample_many_is_an_inference_route(env):
    from shgan_amd import _lib
    G, x, z = env['make'](), env['x'], env['z']
    p = next(G.parameters())
    p.requires_grad_(True)
    with torch.enable_grad():
        with pytest.raises(_lib.ShgError, match='inference route'):
            G.sample_many(x, z, noise_mode='const')
    assert tuple(G.sample_many(x, z, noise_mode='const').shape) == (2, K, 3, 256, 256)            # under no_grad the same module runs
    with pytest.raises(_lib.ShgError, match=r'z must be \[N, K, z_dim\]'):
        G.sample_many(x, z[:, 0])
