"""Host side of pluralistic sampling (K completions per masked input): registry, configs, argument checks, the pair tables of the
diversity measure and the C ABI's new symbols.  On the commit before this feature every test here fails with a missing registry name,
attribute, module or symbol."""
import ctypes
import os
import re

import pytest
import torch

import shgan_amd  # noqa: F401
from conftest import ROOT
from shgan_amd import _lib, configs
from shgan_amd.model_zoo import comodgan, get_model, shgan, stylegan  # noqa: F401  (importing the modules fills the registry)

SMALL = dict(ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128)
NEW = ('shg_plural_expand', 'shg_plural_composite_u8', 'shg_lpips_head_pairs_scratch_bytes', 'shg_lpips_head_pairs_f32')


def test_registry_holds_the_plural_synthesis_with_the_keys_of_synthesis():
    assert 'comodgan_synthesis_plur' in set(get_model().model.keys())
    args = dict(w_dim=64, w0_dim=128, resolution=256, rgb_n=3, ch_base=2048, ch_max=32, use_fp16_after_res=None)
    plur = get_model()(dict(type='comodgan_synthesis_plur', args=args))
    plain = get_model()(dict(type='comodgan_synthesis', args=args))
    assert type(plur) is comodgan.Synthesis_Plur and isinstance(plur, comodgan.Synthesis)
    assert list(plur.state_dict().keys()) == list(plain.state_dict().keys())
    assert [tuple(v.shape) for v in plur.state_dict().values()] == [tuple(v.shape) for v in plain.state_dict().values()]
    plur.load_state_dict(plain.state_dict(), strict=True)


def test_model_cfg_selects_the_synthesis_network():
    assert configs.model_cfg('shgan_g256')['args']['synthesis']['type'] == 'comodgan_synthesis'            # the default stays
    cfg = configs.model_cfg('shgan_g256', synthesis='comodgan_synthesis_plur', **SMALL)
    assert cfg['args']['synthesis']['type'] == 'comodgan_synthesis_plur'
    assert cfg['args']['synthesis']['args'] == configs.model_cfg('shgan_g256', **SMALL)['args']['synthesis']['args']
    with pytest.raises(KeyError, match='comodgan_synthesis_nope'):
        configs.model_cfg('shgan_g256', synthesis='comodgan_synthesis_nope')
    G = configs.build_generator(256, synthesis='comodgan_synthesis_plur', **SMALL)
    G0 = configs.build_generator(256, **SMALL)
    assert type(G.synthesis).__name__ == 'Synthesis_Plur' and list(G.state_dict().keys()) == list(G0.state_dict().keys())


def test_sample_many_refuses_a_z_of_the_wrong_rank():
    G = configs.build_generator(256, **SMALL).eval().requires_grad_(False)
    x = torch.zeros(2, 4, 256, 256)
    for z in (torch.zeros(2, 64), torch.zeros(2, 3, 64, 1), torch.zeros(3, 3, 64), torch.zeros(2, 0, 64)):
        with pytest.raises(_lib.ShgError, match=r'z must be \[N, K, z_dim\]'):
            G.sample_many(x, z)
    for name in ('encode', 'synthesize', 'expand_encoding'):
        assert callable(getattr(G, name))


def test_pair_tables_are_the_unordered_pairs_in_a_fixed_order():
    from shgan_amd import diversity
    assert diversity.pair_table(1) == []
    assert diversity.pair_table(2) == [(0, 1)]
    assert diversity.pair_table(5) == [(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (1, 4), (2, 3), (2, 4), (3, 4)]
    for k in (1, 2, 5):
        t = diversity.pair_table(k)
        assert len(t) == k * (k - 1) // 2 == len(set(t)) and all(0 <= a < b < k for a, b in t)
        ia, ib = diversity.pair_tables(3, k)
        assert ia.dtype == ib.dtype == torch.int32 and ia.shape == ib.shape == (3 * len(t),)
        assert list(zip(ia.tolist(), ib.tolist())) == [(n * k + a, n * k + b) for n in range(3) for a, b in t]        # rows of [N*K, ...]


def test_eval_loop_options_are_checked_on_the_host():
    from shgan_amd import eval_harness as hz
    with pytest.raises(ValueError, match='samples_per_input'):
        hz.EvalLoop(None, 'cpu', 64, 4, samples_per_input=0)
    with pytest.raises(ValueError, match='samples_per_input >= 2'):
        hz.EvalLoop(None, 'cpu', 64, 4, diversity=object())
    with pytest.raises(ValueError, match='step_fn'):
        hz.EvalLoop(None, 'cpu', 64, 4, samples_per_input=2, step_fn=lambda x, z, o: o)
    loop = hz.EvalLoop(None, 'cpu', 64, 4)                                   # K = 1: nothing of the feature exists
    assert loop.samples_per_input == 1 and loop.samples is None and 'diversity' not in loop.evaluators and loop.image_metrics is None
    with pytest.raises(ValueError, match='diversity_value'):
        loop.diversity_value()


def test_header_and_ctypes_table_agree_on_the_new_symbols():
    hdr = open(os.path.join(ROOT, 'include', 'shgan_hip.h')).read()
    declared = set(re.findall(r'\b(shg_[a-z0-9_]+)\s*\(', hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(raw, name), name
    lib = _lib.get_lib()
    assert _lib.ABI_VERSION == 40 and lib.shg_abi_version() == 40                                  # symbols were added, nothing changed
    assert lib.shg_lpips_head_pairs_scratch_bytes.restype == ctypes.c_size_t
    assert lib.shg_lpips_head_pairs_scratch_bytes(7, 15, 15) == lib.shg_lpips_head_scratch_bytes(7, 15, 15) == 7 * 4 * 8
    assert lib.shg_lpips_head_pairs_scratch_bytes(0, 15, 15) == 0
    # the level descriptor has the layout a C compiler gives the header's struct
    m = re.search(r'typedef struct \{\s*const void\* src;\s*void\* dst;\s*long bytes;[^}]*\} shg_expand_level;', hdr)
    assert m, 'shg_expand_level not found in the header'
    E = _lib.ExpandLevel
    assert (ctypes.sizeof(E), E.src.offset, E.dst.offset, E.bytes.offset) == (24, 0, 8, 16)


def test_argument_checks_of_the_new_entry_points_run_on_the_host():
    lib = _lib.get_lib()
    P = ctypes.c_void_p(16)
    err = lambda: lib.shg_last_error().decode()        # noqa: E731
    assert lib.shg_plural_expand(None, 1, 1, 1, 16, None) == -1 and 'null' in err()
    assert lib.shg_plural_expand(P, 0, 1, 1, 16, None) == -1 and lib.shg_plural_expand(P, 1, 1, 0, 16, None) == -1
    assert lib.shg_plural_expand(P, 1, 1, 1, 0, None) == -1 and 'max_bytes' in err()
    assert lib.shg_plural_expand(P, 3, 0, 4, 16, None) == 0                                        # N = 0: nothing to do, nothing launched
    assert lib.shg_plural_composite_u8(None, P, P, 1, 1, 2, 2, None) == -1 and 'null' in err()
    assert lib.shg_plural_composite_u8(P, P, P, 1, 2, 3, 3, None) == -1 and 'multiple of 4' in err()
    assert lib.shg_plural_composite_u8(P, P, P, 1, 0, 2, 2, None) == -1 and 'K must be' in err()
    assert lib.shg_plural_composite_u8(P, P, P, 0, 3, 2, 2, None) == 0
    I = ctypes.c_int * 3
    ok, bad, neg = I(0, 1, 3), I(0, 4, 1), I(0, -1, 1)
    args = lambda a, b: (P, P, P, a, b, P, 4, 3, 8, 2, 2, P, 1 << 10, P, None, None)      # noqa: E731
    assert lib.shg_lpips_head_pairs_f32(*args(ok, bad)) == -1 and 'pair 1 = (1, 4)' in err() and 'outside [0, 4)' in err()
    assert lib.shg_lpips_head_pairs_f32(*args(neg, ok)) == -1 and 'pair 1 = (-1, 1)' in err()
    assert lib.shg_lpips_head_pairs_f32(*args(ok, None)) == -1 and 'both host tables or neither' in err()
    assert lib.shg_lpips_head_pairs_f32(P, P, P, None, None, P, 4, 3, 8, 2, 2, P, 8, P, None, None) == -1 and 'too small' in err()
    assert lib.shg_lpips_head_pairs_f32(P, P, P, None, None, P, 0, 3, 8, 2, 2, P, 1 << 10, P, None, None) == -1
    assert lib.shg_lpips_head_pairs_f32(P, P, P, None, None, P, 4, 70000, 8, 2, 2, P, 1 << 30, P, None, None) == -1 and 'too large' in err()
