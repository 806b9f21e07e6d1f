#!/usr/bin/env python3
"""Golden vectors of the Spectral Hint Unit at other geometries than the shipped 64 / 4: runs the reference's own ``SHU``
(lib/model_zoo/shgan.py:252-336) and, for case G, its whole ``Generator`` on the CPU and writes data only (seeds, parameters, tables
and the reference's outputs) to tests/golden/:

  shu_geometry.npz          cases A, C, D (input 32, 16, 64): parameters and hints
  shu_geometry_128.npz      cases B, E (input 128): parameters and hints
  shu_geometry_tables.npz   Gaussian-split tables and band-weight tables (``_cw``) of A-E
  shu_geometry_g.npz        case G: a 256^2 generator whose SHU reads the 32^2 feature and stops at 8 (image, composite hash)

One file would be natural, but no file in the repository may exceed 1 MiB, so the cases are grouped by size.  Inputs are not stored:
a case's x is ``RandomState(seed).standard_normal(shape)`` in float32, which the test draws again.  Hints of the levels >= 64 are stored
for the channels {0, max(C//2 - 3, 1), C - 1} only; smaller levels are stored in full.  Every case has tail_sigma_mult = 3 and a
conv0.bias ~ N(0, 0.2), so that the ReLU clips.

Runs ONLY where the reference tree exists; nothing here is imported by the product or by the tests.

Usage:  python tools/gen_golden_shu_geometry.py
"""
import hashlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('SHGAN_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden')

for _name in ['torchvision', 'torchvision.models', 'torchvision.transforms', 'pyspng', 'cv2']:
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules['torchvision'].models = sys.modules['torchvision.models']
sys.modules['torchvision'].transforms = sys.modules['torchvision.transforms']
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from lib.model_zoo import comodgan, shgan  # noqa: E402
from oracle import shgan_oracle as orc  # noqa: E402  (only for init_state_dict)

ACT = 'lrelu_agc(alpha=0.2, gain=sqrt_2, clamp=256)'

# id: (batch, channels, input_res, lowest_res, gaussian_at_input_res, freedom, type, seed, file)
CASES = {
    'A': (2, 32, 32, 4, False, [2, 3], 'piecewise_linear', 601, 'shu_geometry'),
    'B': (1, 32, 128, 8, True, [2, 3], 'piecewise_linear', 602, 'shu_geometry_128'),
    'C': (2, 8, 16, 16, False, [3, 2], 'bicubic', 603, 'shu_geometry'),
    'D': (2, 16, 64, 16, False, [2, 3], 'piecewise_linear', 604, 'shu_geometry'),
    'E': (1, 12, 128, 4, False, [2, 3], 'piecewise_linear', 605, 'shu_geometry_128'),
}
G_CFG = dict(resolution=256, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128)
G_SHU = dict(shu_input_res=32, shu_lowest_res=8)
G_SEED = 611


def stored_channels(c):
    return sorted({0, max(c // 2 - 3, 1), c - 1})


def save(name, arrs):
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    print(f'  wrote {path}  ({size / 1024:.1f} KiB)')
    assert size < 1 << 20, 'a committed file must stay under 1 MiB'


def gen_units():
    files = {}
    tables = {}
    for cid, (n, c, size, lowest, gtop, freedom, ftype, seed, fname) in CASES.items():
        out = files.setdefault(fname, {})
        rs = np.random.RandomState(seed)
        x = rs.standard_normal((n, c, size, size)).astype(np.float32)
        shu = shgan.SHU(c, c, freedom, ftype, input_res=size, lowest_res=lowest, tail_sigma_mult=3, gaussian_at_input_res=gtop).eval()
        sd = {'conv0.weight': (rs.standard_normal((2 * c, 2 * c, 1, 1)) / np.sqrt(2 * c)).astype(np.float32),
              'conv0.bias': (rs.standard_normal(2 * c) * 0.2).astype(np.float32),
              'df1.weight': (1 / (2 * c) + rs.standard_normal((2 * c, 2 * c * freedom[0] * freedom[1])) * (0.1 / (2 * c))).astype(np.float32)}
        shu.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        with torch.no_grad():
            y = shu(torch.from_numpy(x))
            y64 = shu.double()(torch.from_numpy(x).double())
        out[f'{cid}__cfg'] = np.array([n, c, size, lowest, int(gtop), freedom[0], freedom[1], seed], np.int64)
        out[f'{cid}__type'] = np.array(ftype)
        for k, v in sd.items():
            out[f'{cid}__sd__{k}'] = v
        keep = stored_channels(c)
        out[f'{cid}__channels'] = np.array(keep, np.int64)
        worst = 0.0
        for r, t in y.items():
            out[f'{cid}__y{r}'] = (t[:, keep] if r >= 64 else t).numpy()
            worst = max(worst, float((t.double() - y64[r]).abs().max() / y64[r].abs().max()))
        print(f'  case {cid}: levels {sorted(y)}, float32 vs float64 of the reference: {worst:.2e} (relative, max norm)')
        for r, t in shu.gaussian_weight_map.items():
            tables[f'{cid}__gauss{r}'] = t.numpy().astype(np.float32)
        tables[f'{cid}__cw'] = shgan.make_cweight(freedom, (size, size // 2 + 1), type=ftype).numpy().astype(np.float32)
    for fname, arrs in files.items():
        save(fname, arrs)
    save('shu_geometry_tables', tables)


def gen_generator():
    from lib.data_factory.ds_ffhq import RandomMask
    c = G_CFG
    mp = comodgan.Mapping(z_dim=c['z_dim'], c_dim=0, w_dim=c['w_dim'], num_ws=14, num_layers=8, embed_features=None, layer_features=None,
                          activation=ACT, lr_multiplier=0.01, w_avg_beta=0.995)
    shu_args = dict(shu_channels=32, shu_df_freedom=[2, 3], shu_df_type='piecewise_linear', shu_input_res=64, shu_lowest_res=4,
                    shu_tail_sigma_mult=3, shu_gaussian_at_input_res=False)
    shu_args.update(G_SHU)
    enc = shgan.Encoder(resolution=256, ic_n=4, oc_n=c['w0_dim'], ch_base=c['ch_base'], ch_max=c['ch_max'], use_fp16_before_res=None,
                        resample_filter=[1, 3, 3, 1], activation=ACT, mbstd_group_size=0, mbstd_c_n=0, c_dim=None, cmap_dim=None,
                        use_dropout=True, has_extra_final_layer=False, **shu_args)
    syn = comodgan.Synthesis(w_dim=c['w_dim'], w0_dim=c['w0_dim'], resolution=256, rgb_n=3, ch_base=c['ch_base'], ch_max=c['ch_max'],
                             use_fp16_after_res=None, resample_filter=[1, 3, 3, 1], activation=ACT)
    G = comodgan.Generator(mp, enc, syn).eval().requires_grad_(False)
    sd = orc.init_state_dict(256, seed=G_SEED, ch_base=c['ch_base'], ch_max=c['ch_max'], w_dim=c['w_dim'], z_dim=c['z_dim'],
                             w0_dim=c['w0_dim'], noise_strength=0.1, bias_std=0.1)
    G.load_state_dict(sd, strict=True)
    rs = np.random.RandomState(G_SEED + 1)
    real_u8 = rs.randint(0, 256, size=(1, 3, 256, 256)).astype(np.uint8)
    z = rs.standard_normal((1, c['z_dim'])).astype(np.float32)
    np.random.seed(G_SEED + 1)
    mask = np.stack([RandomMask(256, [0, 1])]).astype(np.uint8)                     # [1,1,256,256]
    m = torch.from_numpy(mask.astype(np.float32))
    x = torch.cat([m - 0.5, (torch.from_numpy(real_u8.astype(np.float32)) / 127.5 - 1.0) * m], dim=1)
    with torch.no_grad():
        img = G(x=x, z=torch.from_numpy(z), c=torch.zeros(1, 0), noise_mode='const')
        _, feats = G.encoder(x)
    comb_u8 = ((x[:, 1:4] * m + img * (1 - m)) * 127.5 + 127.5).clamp(0, 255).to(torch.uint8)
    save('shu_geometry_g', dict(
        cfg=np.array([256, c['ch_base'], c['ch_max'], c['w_dim'], c['z_dim'], c['w0_dim']], np.int64), seed=np.int64(G_SEED),
        shu_input_res=np.int64(G_SHU['shu_input_res']), shu_lowest_res=np.int64(G_SHU['shu_lowest_res']),
        mask_bits=np.packbits(mask), img_const=img.numpy(), feat8=feats[8].numpy(), feat16=feats[16].numpy(), feat32=feats[32].numpy(),
        known_sha256=np.array(hashlib.sha256((comb_u8 * torch.from_numpy(mask)).numpy().tobytes()).hexdigest())))


if __name__ == '__main__':
    gen_units()
    gen_generator()
