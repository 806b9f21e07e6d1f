#!/usr/bin/env python
"""Golden vector of the pluralistic synthesis network: runs the reference's own ``Synthesis_Plur`` (lib/model_zoo/comodgan.py:491-512) on the
CPU and writes tests/golden/synthesis_plur.npz.  Like tools/gen_golden.py (whose import shim and helpers it uses) it runs only where the
reference tree exists (``SHGAN_REFERENCE``); the fixture it writes is data and is committed.

Shapes, weights and inputs are those of the ``generator_small`` fixture (res 256, ch_base 2048, ch_max 32, w_dim 64, z_dim 64, w0_dim 128;
weights from ``oracle.init_state_dict(seed=21, ...)``, inputs from seed 22, N = 2), so the masked inputs, z and the encoder outputs are the
ones generator_small.npz already holds and the tests regenerate: this file adds only what is new.

    eps            [2,128]   the standard-normal draw the reference's ``torch.randn_like(w0)`` returned (handed to it, then recorded)
    ws             [2,14,64] the mapping's output (as in generator_small.npz)
    xg             [2,128]   the encoder's x_global, the w0 that is perturbed
    w0_plur        [2,128]   w0 + eps * w0 * 1 as the reference computed it
    img0           [3,256,256]    the whole image of input 0
    img1_ds2       [3,128,128]    the image of input 1, every second row and column  (both whole images are 1.5 MB of float32 that does
    sample_idx/val [8192]    flat positions in input 1's whole image and the values    not compress: more than a committed file may have)
    seeds, cfg     the generator_small seeds (weights, inputs) and widths; eps_seed
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (import shim for the reference, build_reference_generator, synth_inputs, assemble_x, save)

torch = gg.torch
EPS_SEED = 23


def gen_synthesis_plur():
    cfg = dict(resolution=256, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128)
    G = gg.build_reference_generator(**cfg)
    sd = gg.orc.init_state_dict(256, seed=21, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128, noise_strength=0.1, bias_std=0.1)
    G.load_state_dict(sd, strict=True)
    plur = gg.comodgan.Synthesis_Plur(w_dim=64, w0_dim=128, resolution=256, rgb_n=3, ch_base=2048, ch_max=32, use_fp16_after_res=None,
                                      resample_filter=[1, 3, 3, 1], activation=gg.ACT).eval().requires_grad_(False)
    assert list(plur.state_dict().keys()) == list(G.synthesis.state_dict().keys())
    plur.load_state_dict(G.synthesis.state_dict(), strict=True)
    real_u8, mask, z = gg.synth_inputs(2, 256, 64, seed=22)
    x = gg.assemble_x(real_u8, mask)
    c = torch.zeros(2, 0)
    eps = torch.randn(2, 128, generator=torch.Generator().manual_seed(EPS_SEED))
    seen = []

    def randn_like(t, *a, **kw):           # the one draw of Synthesis_Plur.forward with noise_mode='const'
        assert tuple(t.shape) == tuple(eps.shape), t.shape
        seen.append(1)
        return eps.clone()
    with torch.no_grad():
        ws = G.mapping(torch.from_numpy(z), c)
        xg, feats = G.encoder(x)
        orig = torch.randn_like
        torch.randn_like = randn_like
        try:
            img = plur(xg, feats, ws, noise_mode='const')
        finally:
            torch.randn_like = orig
    assert len(seen) == 1
    flat = img[1].numpy().reshape(-1)
    idx = np.sort(np.random.RandomState(EPS_SEED).choice(flat.size, 8192, replace=False)).astype(np.int64)
    gg.save('synthesis_plur', eps=eps.numpy(), ws=ws.numpy(), xg=xg.numpy(), w0_plur=(xg + eps * xg * 1).numpy(),
            img0=img[0].numpy(), img1_ds2=img[1, :, ::2, ::2].numpy(), sample_idx=idx, sample_val=flat[idx], seeds=np.array([21, 22], dtype=np.int64),
            eps_seed=np.int64(EPS_SEED), cfg=np.array([256, 2048, 32, 64, 64, 128], dtype=np.int64))


if __name__ == '__main__':
    torch.set_grad_enabled(False)
    gen_synthesis_plur()
