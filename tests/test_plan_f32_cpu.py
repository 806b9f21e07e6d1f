"""The launch plans of the float32 conv / FIR / weight-gradient / optimiser kernels on the host (no GPU): tests/plan_f32.py against the library's
own host-side queries, every case of tests/test_gpu_loop_bounds_fp32.py on its edge and able to see its defect, and the reachability of the
bounds that turned out to have no input.

What the queries can and cannot confirm.  ``shg_conv2d_workspace_bytes``, ``shg_conv2d_wino_workspace_bytes``, ``shg_conv2d_wino4_workspace_bytes``,
``shg_conv2d_wgrad_workspace_bytes`` and ``shg_conv2d_wgrad_wino_workspace_bytes`` return split factor x output bytes, so the restated
tile_search / conv_ksplit (through the tile count), shg_wino_ksplit with both tile plans, wgrad_slices and wgw_slices are held to the library
byte for byte.  No query exposes the tail split of launch_conv (tail_first / tail_ks / tail_ips: the GPU cases assert its TWO launches), the
ragged recomputation ``ksplit = cdiv(I, i_per_slice)`` and the workspace halving (the GPU cases assert the reduction kernel present / absent),
the plane and block caps of upfirdn2d.hip, the item counts of the marching kernels or the optimiser's grid: for those the restatement is read
against the source by the constant scan alone, and a wrong restatement shows as a GPU case that leaves its route or its launch count.  The
up launch of conv_wino_poly.hip is restated and held to ``shg_conv2d_up_poly_workspace_bytes``; its down launch has no split."""
import random

import numpy as np
import pytest
import torch

import shgan_amd  # noqa: F401
from shgan_amd import _lib, optim

import adam_f64
import plan_f32 as P
import test_gpu_loop_bounds_fp32 as T
from conftest import rel_err

C = P.constants()


def test_scan_reads_numbers_and_the_route_tables_instantiations_exist():
    assert all(isinstance(v, int) or (k == 'FIR_UP_TV' and all(isinstance(x, int) for x in v)) or (k == 'WGRAD_BYTES_CAP' and v is None) for k, v in C.items()), C
    assert C['OPT_CHUNK'] == optim.CHUNK
    assert len(P.conv_instantiations()) == 13
    for name in (T.S1_DB, T.S1_NARROW, T.S1_WIDE, T.S2_DB, T.S2_NARROW, T.UP_EPI_W, T.UP_SMALL):
        P.inst(name)
    assert P.inst(T.S1_DB)['DB'] and P.inst(T.S2_DB)['DB'] and P.inst(T.UP_EPI_W)['DB'] and not P.inst(T.S1_NARROW)['DB']
    assert {t[1] for t in P.conv_instantiations()} == {8, 32} and C['WINO_KC'] == C['WINO4_KC'] == C['POLY_KC']


def _named_conv_shapes():
    for name, obj in T.CONV_CASES.items():
        for cus in (T.CUS if callable(obj.size) else (256,)):
            H, W = obj.hw(cus)
            yield obj.N, obj.I, obj.O, H, W, obj.k, obj.mode, obj.pad, 1


def test_plans_equal_the_library_workspace_queries():
    """300 seeded shapes and the shapes of the GPU cases: wherever the library exports a query, the restated plan gives its byte count exactly."""
    lib = _lib.get_lib()
    r = random.Random(20)
    conv = list(_named_conv_shapes())
    wino = [(1, o.I, o.O, o.H, o.W) for o in list(T.WINO_CASES.values()) + list(T.POLY_CASES.values())]
    wg = [(o.N, o.I, o.O, o.H, o.W, o.oh, o.ow, o.k) for o in T.WGRAD_CASES.values()]
    for _ in range(300):
        NB, I, O = r.choice([1, 1, 2, 3, 5, 7, 16]), r.randint(1, 1100), r.choice([3, 16, 32, 64, 65, 128, 200, 256, 512])
        H, W = r.randint(4, 140), r.randint(4, 140)
        k = r.choice([3, 3, 1])
        mode = r.choice([0, 1, 2]) if k == 3 else 0
        conv.append((NB, I, O, H, W, k, mode, r.choice([0, 1]) if mode != 2 else 0, r.choice([1, 1, 2])))
        wino.append((NB, I, O, H, W))
        wg.append((NB, I, O, H, W, H, W, k))
    for NB, I, O, H, W, k, mode, pad, wgr in conv:
        assert int(lib.shg_conv2d_workspace_bytes(NB, I, O, H, W, k, k, mode, pad, wgr)) == P.conv_workspace_bytes(NB, I, O, H, W, k, mode, pad, wgr), \
            (NB, I, O, H, W, k, mode, pad, wgr)
    for NB, I, O, H, W in wino:
        op = P.cdiv(O, 64) * 64
        assert int(lib.shg_conv2d_wino_workspace_bytes(NB, I, O, op, H, W)) == P.wino_workspace_bytes('wino', NB, I, O, op, H, W), (NB, I, O, H, W)
        assert int(lib.shg_conv2d_wino4_workspace_bytes(NB, I, O, op, H, W)) == P.wino_workspace_bytes('wino4', NB, I, O, op, H, W), (NB, I, O, H, W)
        assert int(lib.shg_conv2d_wgrad_wino_workspace_bytes(NB, I, O, H, W)) == P.wgw_plan(NB, I, O, H, W)['ws_bytes'], (NB, I, O, H, W)
        for h, w in ((H, W), (H // 2 * 2, W // 4 * 4)):           # (the polyphase form wants even rows and whole float4 rows)
            assert int(lib.shg_conv2d_up_poly_workspace_bytes(NB, I, O, op, h, w)) == P.up_poly_workspace_bytes(NB, I, O, op, h, w), (NB, I, O, h, w)
            assert bool(lib.shg_conv2d_up_poly_supported(NB, I, O, h, w)) == bool(P.up_poly_supported(NB, I, O, h, w))
    for NB, I, O, H, W, oh, ow, k in wg:
        assert int(lib.shg_conv2d_wgrad_workspace_bytes(NB, I, O, oh, ow, k, k)) == P.wgrad_workspace_bytes(NB, I, O, oh, ow, k), (NB, I, O, oh, ow, k)
    # the split cases of the GPU table ask the library for exactly the slices their plan runs
    for name, o in T.WGRAD_CASES.items():
        p = o.plan()
        got = int(lib.shg_conv2d_wgrad_wino_workspace_bytes(o.N, o.I, o.O, o.H, o.W)) if o.wino else \
            int(lib.shg_conv2d_wgrad_workspace_bytes(o.N, o.I, o.O, o.oh, o.ow, o.k, o.k))
        want = p['nslice'] if o.wino else P.wgrad_slices(o.N, o.I, o.O, o.oh, o.ow, o.k * o.k)
        assert got == want * o.O * o.I * o.k * o.k * 4, name


def _cus_of(obj):
    return T.CUS if (isinstance(obj, T.Conv) and callable(obj.size)) else (256,)


@pytest.mark.parametrize('case', sorted(T.CASES))
def test_case_sits_on_its_edge(case):
    """From constants scanned out of the sources; the CU-dependent shapes at 256 compute units and at what the builder makes of 304 and 128."""
    obj = T.CASES[case]
    shapes = set()
    for cus in _cus_of(obj):
        obj.where(cus)
        if isinstance(obj, T.Conv):
            shapes.add(obj.hw(cus))
    if isinstance(obj, T.Conv) and callable(obj.size):
        assert len(shapes) == len(T.CUS), f'{case}: the builder does not adapt to the CU count: {shapes}'


@pytest.mark.parametrize('case', sorted(T.CASES))
def test_case_sees_its_defect(case):
    """The float64 reference with the edge's contribution removed is at least 100 x the case's tolerance away, in the GPU test's metric (for
    the cropped cases: on the crop)."""
    ref, bad, tol = T.CASES[case].defect(256)
    d = rel_err(bad.numpy().reshape(-1), ref.numpy().reshape(-1))
    assert d >= 100 * tol, f'{case}: the defect stand-in is {d:.2e} from the reference, tolerance {tol:.0e}: the case could not tell them apart'


def test_every_listed_path_has_a_case():
    kinds = {type(o).__name__ for o in T.CASES.values()}
    assert kinds == {'Conv', 'PolyUp', 'Wino', 'FirSame', 'FirDownPlanar', 'FirUpPlanar', 'FirGeneric', 'March', 'Wgrad'}
    assert {o.kern for o in T.CONV_CASES.values() if o.launches == 2} == {T.S1_DB, T.S2_DB, T.UP_EPI_W}       # one DB instantiation per mode splits
    assert {o.kernel.split('<')[0] for o in T.WGRAD_CASES.values()} == {'conv_wgrad_kernel', 'conv_wgrad_full_kernel', 'conv_wgrad_packed_kernel', T.WGW}
    assert {o.kernel.split('<')[0] for o in T.FIR_CASES.values() if isinstance(o, T.March)} == {
        'fir_down_march_kernel', 'fir_down_march4_kernel', 'fir_up_march_kernel', 'fir_dn2_march_kernel', 'fir_up2_march_kernel'}


# ------------------------------------------------------------------------------------------------
# reachability: bounds without an input
# ------------------------------------------------------------------------------------------------

def test_wgrad_partial_sums_never_reach_256_mb():
    """wgrad_slices carried ``s = min(s, 256 MB / bytes per slice)``.  For every I, O <= 4096 and both tap counts the slices it plans without that
    cap hold less than 256 MB, so the cap never changed a result: it is gone from the source (WGRAD_BYTES_CAP None), and this holds the bound."""
    assert C['WGRAD_BYTES_CAP'] is None
    i = np.arange(1, 4097, dtype=np.int64)
    tiles = ((i + 63) // 64)[:, None] * ((i + 63) // 64)[None, :]
    io = i[:, None] * i[None, :]
    worst = 0
    for taps, target in ((9, C['WGRAD_WG']), (1, C['WGRAD_WG_1X1'])):
        s = np.minimum((target + tiles - 1) // tiles, C['WGRAD_MAX_SLICES'])
        bytes_ = np.where(s > 1, s * io * taps * 4, 0)
        worst = max(worst, int(bytes_.max()))
        assert (np.where(s > 1, (256 << 20) // (io * taps * 4), s) >= s).all()           # the removed line never lowered s
    assert worst < 256 << 20
    assert P.wgrad_slices(1, 4096, 4096, 64, 64, 9) == 1 and P.wgrad_slices(8, 64, 64, 512, 512, 9) == C['WGRAD_WG']


def test_wino_split_reduce_cap_reachable_for_f4x4_and_the_polyphase_form_not_for_f2x2():
    """A Winograd launch splits only while tiles * ks < 256, i.e. with fewer than 256 workgroups of 64 channels; wino_split_reduce_kernel runs its
    4096 workgroups x 256 threads x 4 outputs in one trip below 4 194 304 outputs.  F(2x2) tiles hold 16 x 16 or 8 x 32 = 256 pixels: at most
    255 x 64 x 256 outputs, below the cap -- no second trip exists.  F(4x4) tiles hold 512 pixels: reachable, and 'wino4_reduce_second_trip' runs
    it.  The polyphase up launch reduces 4 (H+1) (W+1) outputs per channel from workgroups of 256 input pixels (scheme UB) plus 576 (UA):
    reachable as well, 'poly_up_reduce_second_trip' runs it."""
    one_trip = C['WINO_REDUCE_CAP'] * 256 * 4
    px2 = max(C['WINO_TW_WIDE'] * C['WINO_TH_WIDE'], C['WINO_TW'] * C['WINO_TH'])
    px4 = C['W4_TW'] * C['W4_TH']
    assert (C['WINO_FILL'] - 1) * 64 * px2 < one_trip
    assert (C['WINO_FILL'] - 1) * 64 * px4 > one_trip
    r = random.Random(3)
    for _ in range(2000):                          # and by the plan itself: no split F(2x2) launch has a capped reduction grid with work left over
        NB, I, O, H, W = r.choice([1, 2, 4]), r.choice([128, 256, 512, 1024]), r.choice([64, 128, 256]), r.randint(16, 600), 4 * r.randint(4, 150)
        tiles, nchunk, _ = P.wino_tiles('wino', NB, I, O, H, W)
        if P.wino_ksplit(tiles, nchunk) > 1:
            assert NB * O * H * W <= one_trip, (NB, I, O, H, W)
    o = T.WINO_CASES['wino4_reduce_second_trip']
    assert o.O * o.H * o.W > one_trip and o.plan()['ks'] > 1
    o = T.POLY_CASES['poly_up_reduce_second_trip']
    assert 4 * o.O * (o.H + 1) * (o.W + 1) > one_trip and o.plan()['ks'] > 1 and o.plan()['tiles'] < C['WINO_FILL']


def test_wino_recomputed_slice_count_never_drops():
    """shg_wino_split recomputes ks = cdiv(nchunk, cps) after cps = cdiv(nchunk, ks).  That is smaller than ks only when (ks - 1) * cps >= nchunk,
    i.e. nchunk < ks (ks - 1); shg_wino_ksplit grants ks slices only from nchunk >= 8 * 2 * (ks / 2) = 8 ks chunks and at most 128 chunks exist, and a
    halved ks is smaller still: the recomputation never changes ks (it does for the direct kernels: 'splitk_ragged_fewer_slices')."""
    for tiles in (1, 2, 3, 7, 16, 100, 255):
        for nchunk in range(1, C['WINO_MAX_CHUNKS'] + 1):
            for ws in (10 ** 12, 5, 3, 2):
                p = P.wino_split(tiles, nchunk, 1, ws)
                assert p['ks'] == p['ks_fit'] and 0 < p['last'] <= p['cps'], (tiles, nchunk, ws, p)


def test_tail_split_rules_that_decide():
    """launch_conv splits a tail only when two slices of every tail tile fit the free CUs (tail * 2 <= slots, the first turn of the tk loop), so its
    ``tail * 10 < slots * 6`` is implied and never decides -- the edge the cases sit on is 50 %, and LOWERING the 60 % below 50 % moves
    's1_tail_half_splits_tk2' off its edge.  tail_ips = cdiv(chunks, tk) * KC is not followed by a recomputed slice count (split-K has one), so
    the last of 8 slices can start at or behind channel I (33 ... 35, 41, 42 and 49 chunks): it then multiplies nothing and parks zeros, its
    unconditional first weight fetch stays inside the weights' padding to 32 channels ('s1_tail_tk8_empty_last_slice' runs one)."""
    assert C['TAIL_NUM'] * 1 >= C['TAIL_DEN'] * 1 and C['TAIL_DEN'] * 2 > C['TAIL_NUM']          # 60 % > 50 %
    t = P.inst(T.S1_DB)
    empty = set()
    for slots in (64, 128, 256, 304):
        for tail in range(1, slots):
            for chunks in range(1, 130):
                tk = 1
                while tk < C['TAIL_KS_MAX'] and tail * tk * 2 <= slots and chunks // (tk * 2) >= C['TAIL_MIN_CHUNKS']:
                    tk *= 2
                if tk > 1:
                    assert tail * C['TAIL_NUM'] < slots * C['TAIL_DEN']
                    ips = P.cdiv(chunks, tk) * t['KC']
                    lo = (chunks - 1) * t['KC'] + 1                                      # the fewest channels with this many chunks
                    assert (tk - 1) * ips + t['KC'] <= P.cdiv(lo, 32) * 32               # the last slice's first chunk of weights exists
                    assert (tk - 2) * ips < lo                                           # at most the LAST slice is empty
                    if (tk - 1) * ips >= chunks * t['KC']:
                        empty.add((tk, chunks))
                    assert tail * tk <= slots
    assert empty == {(8, 33), (8, 34), (8, 35), (8, 41), (8, 42), (8, 49)}
    assert C['TAIL_WS'] == 256 * 128 * 256 * 4          # the bound of the query: 256 tile-slices (a device of more CUs gets no half round split)


def test_tile_search_never_picks_a_height_shrunk_tile_nor_the_fallback():
    """tile_search shrinks a candidate's height to the staging capacity and falls back to one row segment when nothing fits.  Over every pairing of
    instantiation and stride conv_dispatch makes, regions of 1 ... 300 columns: a shrunk candidate never has the fewest tiles (the next narrower
    width fits unshrunk), and an 8-column one-row tile always fits, so neither path produces the tile a kernel runs with."""
    pairs = set()
    for O in (32, 128):
        for ohw in ((4, 4), (16, 16), (8, 32), (16, 40)):
            for ins in (False, True):
                pairs.add((P.conv_dispatch(O, ohw[0], ohw[1], 3, 0, in_scale=ins), 1, 3))
                pairs.add((P.conv_dispatch(O, ohw[0], ohw[1], 3, 1, in_scale=ins), 2, 3))
                pairs.add((P.conv_dispatch(O, ohw[0], ohw[1], 1, 0), 1, 1))
                for raw in (False, True):
                    pairs.add((P.conv_dispatch(O, ohw[0], ohw[1], 3, 2, raw_out=raw), 1, 2))
    assert {t for t, _, _ in pairs} == P.conv_instantiations()
    for t, S, span in sorted(pairs):
        ntaps, kc, mo, np_, wo, wp, xq, up, db, occ = t
        BP, cap = np_ * 32 * wp, xq * wo * wp * 64
        for NB in (1, 3):
            for rows in (1, 2, 3, 5, 8, 9, 17, 33, 64):
                for cols in range(1, 301):
                    q = P.tile_search(NB, rows, cols, BP, 1, S, span, span, cap)
                    assert not q['fallback'] and q['TH'] == q['th_unshrunk'], (t, S, NB, rows, cols, q)


# ------------------------------------------------------------------------------------------------
# optimiser
# ------------------------------------------------------------------------------------------------

def test_optimiser_cases_pass_the_grid_cap():
    p = T.opt_plan()
    shapes = T.opt_shapes()
    assert p['chunks'] > C['OPT_MAX_BLOCKS'] == p['grid'] and p['trips'] == 2
    tab = optim.build_adam_table([(4096, 0, 0, int(np.prod(s)), i, 0) for i, s in enumerate(shapes)], [(4096, 4096, 4096, 1 << 40)])
    assert [int(v) for v in tab[:, -1]] == [int(v) for v in p['first']]
    first = T.opt_unstepped()
    big = int(np.argmax([int(np.prod(s)) for s in shapes]))
    assert first[0] is None and first[big] is not None and 0 < first[big] < int(np.prod(shapes[big])) and all(f == 0 for f in first[big + 1:])


def test_optimiser_case_sees_chunks_left_unstepped():
    """One Adam step and one EMA lerp over opt_shapes() in float64, then with everything a second trip of the grid would update left as it was:
    at least 100 x the tolerance (2 x torch-float32's own distance from the float64 yardstick) away."""
    rs = np.random.RandomState(0)
    shapes, first = T.opt_shapes(), T.opt_unstepped()
    worst_tol, dist = 0.0, {}
    for s, f0 in zip(shapes, first):
        p0, g = rs.standard_normal(s).astype(np.float32), rs.standard_normal(s).astype(np.float32)
        y = adam_f64.adam_step_f64(p0.astype(np.float64), g.astype(np.float64), np.zeros(s), np.zeros(s), 0, 0.002, 0.9, 0.999, 1e-8)
        tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
        tp.grad = torch.from_numpy(g)
        opt = torch.optim.Adam([tp], lr=0.002, betas=(0.9, 0.999), eps=1e-8)
        opt.step()
        st = opt.state[tp]
        src = rs.standard_normal(s).astype(np.float32)
        b32 = float(np.float32(0.9))
        ye = adam_f64.ema_f64(p0.astype(np.float64), src, b32)
        te = torch.from_numpy(src).lerp(torch.from_numpy(p0), b32).numpy()
        for key, ours, ref, init in (('p', tp.detach().numpy(), y[0], p0), ('m', st['exp_avg'].numpy(), y[1], np.zeros(s, np.float32)),
                                     ('v', st['exp_avg_sq'].numpy(), y[2], np.zeros(s, np.float32)), ('ema', te, ye, p0)):
            worst_tol = max(worst_tol, 2 * adam_f64.rel_err(ours, ref))
            if f0 is not None:
                bad = np.array(ref, np.float64).reshape(-1).copy()
                bad[f0:] = init.reshape(-1)[f0:]
                dist[key] = min(dist.get(key, 1e9), adam_f64.rel_err(bad, np.asarray(ref, np.float64).reshape(-1)))
    assert set(dist) == {'p', 'm', 'v', 'ema'}
    for key, d in dist.items():
        assert d >= 100 * worst_tol, (key, d, worst_tol)
