"""Loop bounds of the float32 convolution, FIR, weight-gradient and optimiser kernels against float64 (run with -m gpu on an MI355X).

tests/test_gpu_routes_fp32.py puts a case either side of every DISPATCH predicate; the cases here stay on one route and go to the bounds of the
loops inside it: the tail split of the one-workgroup-per-CU direct kernels (a second launch of the same instantiation), ragged and halved K
splits and their grid-stride reductions, the tile shapes of tile_search, second trips of the plane-walking FIR kernels with their prefetched
windows, partial last workgroups of the marching kernels, several chunks per weight-gradient slice with a short last one, and optimiser chunks
past the grid cap.

A case is an object with three faces:
  * ``where(cus)``   host only: asserts, from the launch plan restated in tests/plan_f32.py (constants scanned from the sources), that the case
                     sits on the edge it is named after -- for a device of ``cus`` compute units where the plan depends on them;
  * ``defect(cus)``  host only: (reference, stand-in, tolerance) -- the float64 reference once more with the edge's contribution removed (a K
                     slice dropped, second-trip planes left at the first trip's values, ...); tests/test_plan_f32_cpu.py asserts the stand-in is
                     at least 100 x the tolerance away, so a case that could not see its defect fails before it reaches a GPU;
  * ``run(cus)``     on the GPU: (call, reference, tolerance, expected kernels, forbidden kernels, launch counts, switches).
Tolerances are the project's: TOL_CONV for convolutions and weight gradients, TOL_PW for FIR passes, the 2 x torch-float32 rule of
tests/test_gpu_optim.py for Adam and the EMA.  References that would not fit the time budget whole are evaluated on a CROP: the row bands that hold
every tail (or otherwise special) work item plus the first band of ordinary ones, named in the case (``bands``); the whole output must still be
finite (for the transposed mode's phase planes: the extents the kernel defines, which are compared whole)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import plan_f32 as P
from conftest import rel_err
from route_probe import any_hit, count_of, launch_counts
from test_gpu_routes_fp32 import (MFMA, MSPLIT, S1_DB, S1_NARROW, S1_WIDE, S2_DB, S2_NARROW, TOL_CONV, TOL_PW, UP_EPI_W, UP_SMALL, WINO, WINO4, WSPLIT,
                                  WGW, act64, dev, rnd)

DEV = 'cuda:0'
CUS = (256, 304, 128)            # compute-unit counts the CU-dependent builders are shown to adapt to (the host test); the GPU test asks the device


def _kk():
    import shgan_amd  # noqa: F401
    from shgan_amd import kernels
    return kernels


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------------------------------------
# direct convolution (conv_mfma.hip): tail split, split-K, tile_search
# ------------------------------------------------------------------------------------------------

class Conv:
    """One conv2d call that must run the instantiation ``kern``.  ``size``: (H, W) or a function of the CU count that returns the number of work
    items the shape must produce (the shape is then searched with the restated plan).  ``edge(plan, consts, cus)`` -> the property that puts the
    case on its edge.  ``ws``: None = the workspace kernels.conv2d passes; a function plan -> bytes = the C entry point called directly with a
    workspace of that size.  ``crop``: compare on the bands of the tail work items plus the first band only."""

    def __init__(self, kern, mode, N, I, O, size, edge, k=3, pad=None, offset=0, epi=False, in_scale=False, bias=False, ws=None, crop=False,
                 launches=None, expect=(), forbid=(), switches=None, search_w=(64, 96, 72, 40), drop='tail', groups=1):
        self.kern, self.mode, self.N, self.I, self.O, self.size, self.edge, self.k = kern, mode, N, I, O, size, edge, k
        self.pad = (1 if (mode == 0 and k == 3) else 0) if pad is None else pad
        self.offset, self.epi, self.in_scale, self.bias, self.ws, self.crop = offset, epi, in_scale or epi, bias or epi, ws, crop
        self.launches, self.expect, self.forbid, self.switches = launches, tuple(expect), tuple(forbid), dict(switches or {})
        self.search_w, self.drop, self.groups = search_w, drop, groups        # groups > 1: per-slot weights, image n uses group n % groups
        self.t = P.inst(kern)

    # -- shape and plan ---------------------------------------------------------------------------
    def _plan_hw(self, H, W, cus, ws='auto'):
        wsb = None
        if ws == 'auto' and self.ws is not None:
            wsb = self.ws(self._plan_hw(H, W, cus, ws=None))
        return P.conv_plan(self.N, self.I, self.O, H, W, self.k, self.mode, self.pad, self.t, cus, ws_bytes=wsb, wgroups=self.groups)

    def hw(self, cus):
        if not callable(self.size):
            return self.size
        target = self.size(cus)
        per_img = self.t['BP'] * target // (self.N * P.cdiv(self.O, self.t['BO']))         # output pixels per image, roughly
        best = None
        for W in self.search_w:
            ow = W if self.mode != 1 else (W - 3) // 2 + 1
            h0 = per_img // max(ow, 1)
            for oh in range(max(h0 - 24, 8), h0 + 25):
                H = oh if self.mode != 1 else 2 * oh + 1
                if self._plan_hw(H, W, cus, ws=None)['nwork'] == target and (best is None or H * W < best[0] * best[1]):
                    best = (H, W)
        assert best is not None, f'no shape with {target} work items found for {self.kern}'
        return best

    def plan(self, cus):
        H, W = self.hw(cus)
        return self._plan_hw(H, W, cus)

    def where(self, cus):
        H, W = self.hw(cus)
        p = self.plan(cus)
        OHp, OWp, _, _ = P.conv_geometry(H, W, self.k, self.mode, self.pad)
        raw = self.mode == 2 and not (self.bias or self.epi)
        assert P.conv_dispatch(self.O, OHp, OWp, self.k, self.mode, wgroups=self.groups, in_scale=self.in_scale, raw_out=raw) == self.t['args'], (self.kern, H, W)
        assert self.edge(p, P.constants(), cus), f'{self.kern} at {self.N}x{self.I}->{self.O}x{H}x{W}, {cus} CUs: no longer on its edge: ' + str(
            {k: v for k, v in p.items() if k != 'cls'}) + str([(q['TW'], q['TH'], q['TN'], q['n_tiles']) for q in p['cls']])
        if self.launches is not None:
            assert p['launches'] == self.launches, (p['launches'], self.launches)
        assert (p['reduce_grid'] > 0) == (MSPLIT in self.expect), 'split-K reduction expected exactly where the plan splits'
        assert max(self.N * self.I * H * W, p['out_elems']) * 4 < 300 << 20
        return p

    # -- tensors and float64 references -------------------------------------------------------------
    def tensors(self, cus):
        H, W = self.hw(cus)
        N, I, O, k = self.N, self.I, self.O, self.k
        OHp, OWp, _, _ = P.conv_geometry(H, W, k, self.mode, self.pad)
        oh, ow = (2 * H + 1, 2 * W + 1) if self.mode == 2 else (OHp, OWp)
        t = dict(x=rnd(101, N, I, H, W), w=rnd(102, self.groups * O, I, k, k), g=1.0 / np.sqrt(I * k * k), H=H, W=W, oh=oh, ow=ow)
        t['in_scale'] = rnd(103, N, I, lo=0.5) if self.in_scale else None
        t['bias'] = rnd(104, O) if self.bias else None
        if self.epi:
            t['out_scale'], t['noise'] = rnd(105, N, O, lo=0.5), rnd(106, N, 1, oh, ow)
            t['residual'] = rnd(107, N, O, oh, ow)
        return t

    def bands(self, cus):
        """Row bands (n0, n1, r0, r1) of the launch grid that are compared: everything, or (crop) the first tile row and the tail work items."""
        p = self.plan(cus)
        OHp = p['cls'][0]['rows']
        if not self.crop or self.mode == 2:
            return [(0, self.N, 0, OHp)]
        out = {}
        for wk in range(min(p['tail_first'], p['nwork'] - 1), p['nwork']):         # (no tail: the last work item)
            _, _, n0, n1, y0, y1, _, _, _ = P.work_rect(p, wk)
            b = out.setdefault((n0, n1), [y0, y1])
            b[0], b[1] = min(b[0], y0), max(b[1], y1)
        first = (0, p['cls'][0]['TN'], 0, p['cls'][0]['TH'])                        # the first tile row of ordinary work items
        res = [(n0, n1, a, b) for (n0, n1), (a, b) in sorted(out.items())]
        return ([first] if not any(n0 == 0 and a < first[3] for n0, n1, a, b in res) else []) + res

    def _sums(self, t, band, i_lo=0, i_hi=None):
        """float64 convolution sums over input channels [i_lo, i_hi) on one band (before the layer tail)."""
        n0, n1, r0, r1 = band
        i_hi = self.I if i_hi is None else min(i_hi, self.I)
        x = t['x'][n0:n1, i_lo:i_hi].double()
        if t['in_scale'] is not None:
            x = x * t['in_scale'][n0:n1, i_lo:i_hi].double()[:, :, None, None]
        w = t['w'][:, i_lo:i_hi].double() * t['g']
        if self.groups > 1 and i_hi > i_lo:
            assert self.mode == 0
            return torch.cat([F.conv2d(F.pad(x[j:j + 1, :, max(r0 - 1, 0):r1 + 1], [1, 1, int(r0 == 0), max(r1 + 1 - t['H'], 0)]),
                                       w[((n0 + j) % self.groups) * self.O:((n0 + j) % self.groups + 1) * self.O]) for j in range(n1 - n0)])
        if i_hi <= i_lo:
            return torch.zeros(n1 - n0, self.O, *((t['oh'], t['ow']) if self.mode == 2 else (r1 - r0, t['ow'])), dtype=torch.float64)
        if self.mode == 2:
            return F.conv_transpose2d(x, w.transpose(0, 1), stride=2)
        S, pad, k = (1 if self.mode == 0 else 2), self.pad, self.k
        a, b = r0 * S - pad, (r1 - 1) * S - pad + k               # input rows [a, b)
        xs = x[:, :, max(a, 0):min(b, t['H'])]
        xs = F.pad(xs, [pad, pad, max(-a, 0), max(b - t['H'], 0)])
        return F.conv2d(xs, w, stride=S)

    def _tail(self, t, z, band):
        n0, n1, r0, r1 = band
        sl = (slice(n0, n1), slice(None), slice(None) if self.mode == 2 else slice(r0, r1))
        if self.epi:
            z = z * t['out_scale'][n0:n1].double()[:, :, None, None] + t['noise'][sl].double() * 0.3
        if t['bias'] is not None:
            z = z + t['bias'].double().view(1, -1, 1, 1)
        z = act64(z, self.epi, gain=0.7 if self.epi else 1.0)
        if self.epi:
            z = z + t['residual'][sl].double()
        return z

    def _flat(self, t, zs):
        """Band results -> one vector; the transposed conv's image as the valid extents of its four phase planes (what ``run`` compares)."""
        if self.mode == 2:
            return torch.cat([zs[0][:, :, a::2, c::2].reshape(-1) for a in range(2) for c in range(2)])
        return torch.cat([z.reshape(-1) for z in zs])

    def reference(self, cus, t=None):
        t = self.tensors(cus) if t is None else t
        return self._flat(t, [self._tail(t, self._sums(t, b), b) for b in self.bands(cus)])

    def defect(self, cus):
        """The reference with the edge's contribution removed: drop='tail' -- the tail work items' outputs from their first K slice only (the fix
        launch summing one slice); 'kslice' -- the last split-K slice never added; 'reduce' -- outputs past the first trip of splitk_reduce's
        grid left unwritten; 'tile' -- the ragged last tile column / row / image group left unwritten; None (a case on the far side of an
        edge, which runs without the special path) -- the last work item left unwritten."""
        t, p = self.tensors(cus), self.plan(cus)
        bands = self.bands(cus)
        good = [self._sums(t, b) for b in bands]
        bad = [z.clone() for z in good]
        if self.drop == 'tail':
            assert p['n_tail'] > 0
            for bi, b in enumerate(bands):
                part = self._sums(t, b, 0, p['tail_ips'])
                for wk in range(p['tail_first'], p['nwork']):
                    o0, o1, n0, n1, y0, y1, x0, x1, ci = P.work_rect(p, wk)
                    if self.mode == 2:             # phase-grid rectangle (u, v) -> image pixels 2u + a, 2v + c
                        ys, xs = slice(2 * y0, min(2 * y1, t['oh'])), slice(2 * x0, min(2 * x1, t['ow']))
                        bad[bi][n0:n1, o0:o1, ys, xs] = part[n0:n1, o0:o1, ys, xs]
                    elif n0 >= b[0] and n1 <= b[1] and y0 >= b[2] and y1 <= b[3]:
                        bad[bi][n0 - b[0]:n1 - b[0], o0:o1, y0 - b[2]:y1 - b[2], x0:x1] = part[n0 - b[0]:n1 - b[0], o0:o1, y0 - b[2]:y1 - b[2], x0:x1]
        elif self.drop == 'kslice':
            assert p['ksplit'] > 1
            bad = [self._sums(t, b, 0, (p['ksplit'] - 1) * p['i_per_slice']) for b in bands]
        elif self.drop == 'reduce':
            assert p['reduce_grid'] * 256 < p['out_elems']
            bad[0].view(-1)[p['reduce_grid'] * 256:] = 0.0
        elif self.drop is None:                    # a case that runs WITHOUT the special path: its last work item left unwritten
            o0, o1, n0, n1, y0, y1, x0, x1, ci = P.work_rect(p, p['nwork'] - 1)
            if self.mode == 2:
                bad[0][n0:n1, o0:o1, 2 * y0:2 * y1, 2 * x0:2 * x1] = 0.0
            else:
                b = bands[-1]
                bad[-1][n0 - b[0]:n1 - b[0], o0:o1, y0 - b[2]:y1 - b[2], x0:x1] = 0.0
        else:
            assert self.drop == 'tile'
            q = p['cls'][0]
            if q['cols'] % q['TW']:
                bad[0][:, :, :, q['cols'] - q['cols'] % q['TW']:] = 0.0
            if q['rows'] % q['TH']:
                bad[0][:, :, q['rows'] - q['rows'] % q['TH']:] = 0.0
            if self.N % q['TN']:
                bad[0][self.N - self.N % q['TN']:] = 0.0
        fin = lambda zs: self._flat(t, [self._tail(t, z, b) for z, b in zip(zs, bands)])
        return fin(good), fin(bad), TOL_CONV

    # -- the GPU side -----------------------------------------------------------------------------
    def run(self, cus):
        kk = _kk()
        t, p, bands = self.tensors(cus), self.plan(cus), self.bands(cus)
        H, W, N, O = t['H'], t['W'], self.N, self.O
        ref = self.reference(cus, t)
        xd, pw = dev(t['x'], self.offset), kk.conv_weight_prep(t['w'].to(DEV), gain=t['g'], groups=self.groups)
        d = {k: dev(t.get(k)) for k in ('in_scale', 'out_scale', 'bias', 'noise', 'residual')}
        kw = dict(mode=self.mode, pad=self.pad, in_scale=d['in_scale'], out_scale=d['out_scale'], bias=d['bias'], noise=d['noise'], noise_strength=0.3,
                  act=self.epi, gain=0.7 if self.epi else 1.0, residual=d['residual'])
        if self.mode == 2:
            kw.update(planar=True)
            kw.pop('pad')
        ws = torch.empty(max(p['ws_bytes'] // 4, 1), device=DEV) if self.ws is not None else None

        def raw():
            """kernels.conv2d's call of shg_conv2d_f32 with a workspace of our own size."""
            from shgan_amd import _lib
            y = torch.empty(N, O, t['oh'], t['ow'], device=DEV)
            a, al, g, cl = kk._act_args(self.epi, 0.7 if self.epi else 1.0)
            nz = d['noise']
            rc = _lib.get_lib().shg_conv2d_f32(_p(xd), _p(pw.wt), _p(y), N, self.I, O, pw.op, H, W, self.k, self.k, self.mode, self.pad, 1,
                                               pw.wt.shape[1], _p(d['in_scale']), _p(d['out_scale']), _p(d['bias']), _p(nz),
                                               (2 if N > 1 else 1) if nz is not None else 0, 0.3, a, al, g, cl, _p(d['residual']), 0,
                                               _p(ws) if p['ws_bytes'] else None, p['ws_bytes'], _stream())
            assert rc == 0, rc
            return y

        def call():
            y = raw() if self.ws is not None else kk.conv2d(xd, pw, **kw)
            if self.mode == 2:
                # (the phase planes are [H+1, W+1] from an uninitialised allocation; the kernel defines rows u <= H - a and columns v <= W - c of
                # plane (a, c) only, so that is all a check may read -- the whole of it is compared below, finiteness included)
                return torch.cat([y[a * 2 + c][:, :, :H + 1 - a, :W + 1 - c].reshape(-1) for a in range(2) for c in range(2)])
            assert torch.isfinite(y).all(), 'the whole output must be finite'
            return torch.cat([y[n0:n1, :, r0:r1].reshape(-1) for n0, n1, r0, r1 in bands])
        counts = {self.kern: p['launches']}
        return call, ref, TOL_CONV, (self.kern,) + self.expect, self.forbid, counts, self.switches


def _tail(split, tk=None, ips_ragged=False):
    def edge(p, c, cus):
        ok = p['nwork'] > cus and p['ksplit'] == 1
        if not split:
            return ok and p['n_tail'] == 0 and p['tail'] > 0
        ok = ok and p['n_tail'] == p['tail'] > 0 and p['tail_ks'] == tk and p['launches'] == 2 and p['grid'] == p['tail_first'] + p['tail'] * tk
        return ok and (not ips_ragged or (p['tail_ks'] * p['tail_ips'] > p['chunks'] * 8 and (tk - 1) * p['tail_ips'] < p['chunks'] * 8
                                           and p['chunks'] * 8 > ips_ragged))
    return edge


def _tk_stops_at_tail(p, c, cus):          # the next doubling is refused by tail * tk * 2 <= slots, not by the chunk guard or the cap of 8
    tk = p['tail_ks']
    return _tail(True, tk)(p, c, cus) and tk < c['TAIL_KS_MAX'] and p['tail'] * tk * 2 > cus and p['chunks'] // (tk * 2) >= c['TAIL_MIN_CHUNKS']


def _tk_stops_at_chunks(p, c, cus):        # ... by chunks / (tk * 2) >= 4 alone
    tk = p['tail_ks']
    return _tail(True, tk)(p, c, cus) and tk < c['TAIL_KS_MAX'] and p['tail'] * tk * 2 <= cus and p['chunks'] // (tk * 2) < c['TAIL_MIN_CHUNKS']


def _tk_at_cap(p, c, cus):
    return _tail(True, c['TAIL_KS_MAX'])(p, c, cus) and p['tail'] * p['tail_ks'] * 2 <= cus and p['chunks'] // (p['tail_ks'] * 2) >= c['TAIL_MIN_CHUNKS']


def _no_split_chunks(p, c, cus):           # a small tail, but too few chunks for even two slices: one launch
    return p['nwork'] > cus and 0 < p['tail'] * 2 <= cus and p['chunks'] // 2 < c['TAIL_MIN_CHUNKS'] and p['n_tail'] == 0


def _splitk(**want):
    def edge(p, c, cus):
        return p['ksplit'] > 1 and all(p[k] == v for k, v in want.items())
    return edge


def _tiles(pred):
    return lambda p, c, cus: pred(p['cls'], p)


NOWINO = (WINO, WINO4)

CONV_CASES = {
    # ---- tail split, stride-1 128 x 256 tiles (x through an offset view keeps the layer off the Winograd kernels).  The launch splits only when
    # tail * 2 <= slots (two slices must fit the free CUs), so its "tail * 10 < slots * 6" never decides (test_plan_f32_cpu.py): the edge is 50 %
    's1_full_round_no_tail': Conv(S1_DB, 0, 1, 64, 128, lambda cu: 2 * cu, lambda p, c, cu: p['tail'] == 0 and p['nwork'] == 2 * cu and p['n_tail'] == 0,
                                  offset=1, launches=1, forbid=NOWINO, crop=True, drop=None),
    's1_tail_half_splits_tk2': Conv(S1_DB, 0, 1, 64, 128, lambda cu: cu + cu // 2, _tail(True, 2), offset=1, launches=2, forbid=NOWINO),
    's1_tail_half_plus_one_unsplit': Conv(S1_DB, 0, 1, 64, 128, lambda cu: cu + cu // 2 + 1, _tail(False), offset=1, launches=1, forbid=NOWINO,
                                          crop=True, drop=None),
    's1_tail_tk4_limited_by_tail': Conv(S1_DB, 0, 1, 256, 128, lambda cu: cu + cu // 8 + 1, _tk_stops_at_tail, offset=1, launches=2, forbid=NOWINO, crop=True),
    's1_tail_tk8_at_cap': Conv(S1_DB, 0, 1, 512, 128, lambda cu: cu + cu // 16, _tk_at_cap, offset=1, launches=2, forbid=NOWINO, crop=True),
    # 33 chunks in 8 slices of 5: the last slice starts behind the last channel and multiplies nothing
    's1_tail_tk8_empty_last_slice': Conv(S1_DB, 0, 1, 260, 128, lambda cu: cu + cu // 16, lambda p, c, cu: _tail(True, 8)(p, c, cu)
                                         and 7 * p['tail_ips'] >= 260 > 6 * p['tail_ips'], offset=1, launches=2, forbid=NOWINO, crop=True),
    's1_tail_tk2_limited_by_chunks': Conv(S1_DB, 0, 1, 64, 128, lambda cu: cu + cu // 16, _tk_stops_at_chunks, offset=1, launches=2, forbid=NOWINO, crop=True),
    's1_tail_7_chunks_unsplit': Conv(S1_DB, 0, 1, 56, 128, lambda cu: cu + cu // 16, _no_split_chunks, offset=1, launches=1, forbid=NOWINO, crop=True,
                                     drop=None),
    's1_tail_ragged_last_slice': Conv(S1_DB, 0, 1, 100, 128, lambda cu: cu + cu // 16, _tail(True, 2, ips_ragged=56), offset=1, launches=2, forbid=NOWINO,
                                      crop=True),
    's1_tail_full_layer_tail': Conv(S1_DB, 0, 2, 64, 128, lambda cu: cu + cu // 4, _tail(True, 2), offset=1, epi=True, launches=2, forbid=NOWINO, crop=True),
    # ---- tail split, stride-2 16-wave kernel and the transposed kernel (three tile classes, four phase accumulators, bias in the fix launch)
    # (a quarter round: at more than 256 CUs the tail workspace bound of shg_conv2d_workspace_bytes, 256 tile-slices, holds no half round)
    's2_tail_quarter_splits': Conv(S2_DB, 1, 1, 64, 128, lambda cu: cu + cu // 4, _tail(True, 2), bias=True, launches=2, search_w=(129, 65, 193), crop=True),
    's2_tail_half_plus_one_unsplit': Conv(S2_DB, 1, 1, 64, 128, lambda cu: cu + cu // 2 + 1, _tail(False), bias=True, launches=1, search_w=(129, 65, 193),
                                          crop=True, drop=None),
    'up_tail_splits': Conv(UP_EPI_W, 2, 1, 64, 128, lambda cu: cu + cu // 4, _tail(True, 2), bias=True, launches=2, search_w=(64, 96, 80, 48),
                           forbid=('conv_poly_up_kernel',)),
    'up_tail_half_plus_one_unsplit': Conv(UP_EPI_W, 2, 1, 64, 128, lambda cu: cu + cu // 2 + 1, _tail(False), bias=True, launches=1,
                                          search_w=(64, 96, 80, 48), forbid=('conv_poly_up_kernel',), drop=None),
    # ---- split-K of the single-buffer kernels
    'splitk_ragged_fewer_slices': Conv(S1_NARROW, 0, 1, 259, 32, (15, 16), lambda p, c, cu: p['ksplit'] < p['ks'] and p['chunks'] % p['ks'] != 0
                                       and 259 % 8 != 0 and 259 - (p['ksplit'] - 1) * p['i_per_slice'] < p['i_per_slice'], expect=(MSPLIT,),
                                       forbid=NOWINO, drop='kslice'),
    'splitk_workspace_half': Conv(S1_NARROW, 0, 1, 256, 32, (15, 16), lambda p, c, cu: p['halvings'] == 1 and p['ksplit'] == p['ks_planned'] // 2 > 1,
                                  ws=lambda p: p['ks_planned'] * p['out_elems'] * 4 // 2, expect=(MSPLIT,), forbid=NOWINO, drop='kslice'),
    'splitk_workspace_one_slice': Conv(S1_NARROW, 0, 1, 256, 32, (15, 16), lambda p, c, cu: p['halvings'] >= 2 and p['ks'] == 1 and p['ksplit'] == 1
                                       and p['ks_planned'] >= 4, ws=lambda p: p['out_elems'] * 4, forbid=NOWINO + (MSPLIT,), drop=None),
    'splitk_in_scale_tn2': Conv(S1_NARROW, 0, 3, 256, 32, (7, 10), lambda p, c, cu: p['ksplit'] > 1 and p['tn_max'] > 1, in_scale=True, bias=True,
                                expect=(MSPLIT,), forbid=NOWINO, drop='kslice'),
    'splitk_reduce_second_trip': Conv(S1_NARROW, 0, 1, 64, 64, (93, 98), lambda p, c, cu: p['ksplit'] == 2 and p['out_elems'] > c['SPLITK_REDUCE_CAP'] * 256
                                      and p['out_elems'] % 256 != 0 and p['reduce_grid'] == c['SPLITK_REDUCE_CAP'], bias=True, expect=(MSPLIT,),
                                      forbid=NOWINO, drop='reduce'),
    # ---- tile_search: several images per tile with a ragged last tile (4x4: tn shrunk to the staging capacity), ragged rows and columns, short
    # rows.  (A tile whose HEIGHT was shrunk to the staging capacity is never the chosen one, nor is the fallback: test_plan_f32_cpu.py)
    'tiles_tn_ragged_4x4': Conv(S1_NARROW, 0, 22, 16, 32, (4, 4), _tiles(lambda q, p: q[0]['TN'] > 1 and 22 % q[0]['TN'] != 0 and q[0]['TN'] < 256 // 16), bias=True,
                                forbid=NOWINO + (MSPLIT,), drop='tile'),
    'tiles_tn_ragged_5x7': Conv(S1_NARROW, 0, 11, 16, 32, (5, 7), _tiles(lambda q, p: q[0]['TN'] > 1 and 11 % q[0]['TN'] != 0 and q[0]['TW'] == 7 < 8),
                                bias=True, forbid=NOWINO + (MSPLIT,), drop='tile'),
    'tiles_tn_ragged_down_8x8': Conv(S2_NARROW, 1, 5, 16, 32, (17, 17), _tiles(lambda q, p: q[0]['TN'] > 1 and 5 % q[0]['TN'] != 0), bias=True,
                                     forbid=(MSPLIT,), drop='tile'),
    'tiles_wide_down_ragged': Conv(S2_NARROW, 1, 1, 16, 32, (59, 67), _tiles(lambda q, p: q[0]['rows'] % q[0]['TH'] != 0 and q[0]['cols'] % q[0]['TW'] != 0
                                   and q[0]['tiles_x'] > 1), bias=True, drop='tile'),
    'tiles_ragged_rows_and_cols': Conv(S1_WIDE, 0, 1, 16, 128, (17, 22), _tiles(lambda q, p: q[0]['rows'] % q[0]['TH'] != 0 and q[0]['cols'] % q[0]['TW'] != 0),
                                       bias=True, forbid=NOWINO, drop='tile'),
    'tiles_wgroups_one_image_per_tile': Conv(S1_NARROW, 0, 6, 16, 32, (4, 4), lambda p, c, cu: p['cls'][0]['TN'] == 1 and p['nwork'] == 6 and P.conv_plan(
        6, 16, 32, 4, 4, 3, 0, 1, P.inst(S1_NARROW), cu)['cls'][0]['TN'] > 1, bias=True, groups=3, forbid=NOWINO + (MSPLIT,), drop=None),
    'tiles_up_three_classes_ragged': Conv(UP_SMALL, 2, 5, 16, 32, (5, 7), _tiles(lambda q, p: all(t['n_tiles'] > 0 for t in q) and q[0]['TN'] > 1
                                          and 5 % q[0]['TN'] != 0 and q[2]['TW'] == 1), bias=True, forbid=('conv_poly_up_kernel',), drop=None),
}


# ------------------------------------------------------------------------------------------------
# Winograd K split (wino_common.h): F(2x2) and F(4x4)
# ------------------------------------------------------------------------------------------------

class Wino:
    def __init__(self, kind, I, O, H, W, edge, ws=None, res=None, split=True, drop='kslice'):
        self.kind, self.I, self.O, self.H, self.W, self.edge, self.ws, self.res, self.split, self.drop = kind, I, O, H, W, edge, ws, res, split, drop

    def plan(self):
        op = P.cdiv(self.O, 64) * 64
        tiles, nchunk, kc = P.wino_tiles(self.kind, 1, self.I, op, self.H, self.W)
        out_bytes = self.O * self.H * self.W * 4
        full = P.wino_workspace_bytes(self.kind, 1, self.I, self.O, op, self.H, self.W)
        wsb = full if self.ws is None else self.ws(full)
        p = P.wino_split(tiles, nchunk, out_bytes, wsb, aligned16=self.res != 'offset8')
        p.update(tiles=tiles, nchunk=nchunk, KC=kc, ws_bytes=wsb, out_bytes=out_bytes)
        return p

    def where(self, cus=None):
        p, c = self.plan(), P.constants()
        assert self.H >= (32 if self.kind == 'wino4' else 16) and self.W % 4 == 0 and self.I <= 1024
        assert self.edge(p, c), f'{self.kind} {self.I}->{self.O} {self.H}x{self.W}: no longer on its edge: {p}'
        assert (p['ks'] > 1) == self.split
        return p

    def tensors(self):
        t = dict(x=rnd(111, 1, self.I, self.H, self.W), w=rnd(112, self.O, self.I, 3, 3), b=rnd(113, self.O), g=1.0 / np.sqrt(self.I * 9))
        t['res'] = rnd(114, 1, self.O, self.H, self.W) if self.res else None
        return t

    def _ref(self, t, i_hi=None):
        z = F.conv2d(t['x'][:, :i_hi].double(), t['w'][:, :i_hi].double() * t['g'], padding=1) + t['b'].double().view(1, -1, 1, 1)
        z = act64(z, True, gain=0.7)
        return z + t['res'].double() if t['res'] is not None else z

    def defect(self, cus=None):
        """The last K slice never added (split cases); for the unsplit cases the stand-in drops the last chunk of channels."""
        t, p = self.tensors(), self.plan()
        if self.drop == 'reduce':              # outputs past the first trip of the reduction's grid left at the raw sums' place: unwritten
            ref = self._ref(t)
            bad = ref.clone()
            bad.view(-1)[P.wino_reduce_grid(1, self.O, self.H, self.W) * 1024:] = 0.0
            return ref, bad, TOL_CONV
        keep = (p['ks'] - 1) * p['cps'] * p['KC'] if p['ks'] > 1 else (p['nchunk'] - 1) * p['KC']
        return self._ref(t), self._ref(t, keep), TOL_CONV

    def run(self, cus=None):
        kk = _kk()
        from shgan_amd import _lib
        t, p = self.tensors(), self.plan()
        ref = self._ref(t)
        xd, pw, bd = dev(t['x']), kk.conv_weight_prep(t['w'].to(DEV), gain=t['g']), dev(t['b'])
        rd = dev(t['res'], 2 if self.res == 'offset8' else 0)
        if rd is not None and self.res == 'offset8':
            assert rd.data_ptr() % 16 == 8
        kern = f'{WINO4}' if self.kind == 'wino4' else f'{WINO}'
        if self.ws is None:
            call = lambda: kk.conv2d(xd, pw, mode=kk.MODE_SAME, pad=1, bias=bd, act=True, gain=0.7, residual=rd)
        else:
            ws = torch.empty(max(p['ws_bytes'] // 4, 4), device=DEV)
            lib = _lib.get_lib()
            a, al, g, cl = kk._act_args(True, 0.7)

            def call():
                y = torch.empty(1, self.O, self.H, self.W, device=DEV)
                if self.kind == 'wino4':
                    rc = lib.shg_conv2d_wino4_route_f32(_p(xd), _p(pw.wino4()), _p(y), 1, self.I, self.O, pw.op, self.H, self.W, None, None, _p(bd), None, 0,
                                                        0.0, a, al, g, cl, _p(rd), 0, _p(ws), p['ws_bytes'], _stream())
                else:
                    rc = lib.shg_conv2d_wino_ws_f32(_p(xd), _p(pw.wino()), _p(y), 1, self.I, self.O, pw.op, self.H, self.W, None, None, _p(bd), None, 0,
                                                    0.0, a, al, g, cl, _p(rd), _p(ws), p['ws_bytes'], _stream())
                assert rc == 0, rc
                return y
        expect = (kern, WSPLIT) if self.split else (kern,)
        forbid = (MFMA,) + (() if self.split else (WSPLIT,))
        return call, ref, TOL_CONV, expect, forbid, {}, {}


def _wsplit(ragged=False, halved=0):
    def edge(p, c):
        ok = p['ks'] > 1 and p['halvings'] == halved
        if ragged:
            ok = ok and p['nchunk'] % p['ks_fit'] != 0 and p['last'] < p['cps']
        return ok
    return edge


class PolyUp:
    """conv_poly_up_kernel (the planar transposed convolution without tail operands) through the K split of wino_common.h.  conv_poly_down has no
    split: shg_conv2d_down_poly_f32 takes no workspace (plan_f32's scan holds that conv_wino_poly.hip calls shg_wino_split once)."""

    def __init__(self, I, O, H, W, edge, ws=None, drop='kslice'):
        self.I, self.O, self.H, self.W, self.edge, self.ws, self.drop = I, O, H, W, edge, ws, drop

    def plan(self):
        op = P.cdiv(self.O, 64) * 64
        tiles, nchunk, kc = P.up_poly_tiles(1, self.I, op, self.H, self.W)
        out_bytes = 4 * self.O * (self.H + 1) * (self.W + 1) * 4
        full = P.up_poly_workspace_bytes(1, self.I, self.O, op, self.H, self.W)
        wsb = full if self.ws is None else self.ws(full)
        p = P.wino_split(tiles, nchunk, out_bytes, wsb)
        p.update(tiles=tiles, nchunk=nchunk, KC=kc, ws_bytes=wsb, out_bytes=out_bytes, reduce_grid=P.wino_reduce_grid(4, self.O, self.H + 1, self.W + 1))
        return p

    def where(self, cus=None):
        p = self.plan()
        assert P.up_poly_supported(1, self.I, self.O, self.H, self.W)
        assert p['ks'] > 1 and self.edge(p, P.constants()), f'conv_poly_up {self.I}->{self.O} {self.H}x{self.W}: no longer on its edge: {p}'
        return p

    def tensors(self):
        return dict(x=rnd(171, 1, self.I, self.H, self.W), w=rnd(172, self.O, self.I, 3, 3), g=1.0 / np.sqrt(self.I * 9))

    def _planes(self, t, i_hi=None):
        """The four phase planes [4, 1, O, H+1, W+1] in float64, entries outside a plane's extent zero."""
        full = F.conv_transpose2d(t['x'][:, :i_hi].double(), (t['w'][:, :i_hi].double() * t['g']).transpose(0, 1), stride=2)
        y = torch.zeros(4, 1, self.O, self.H + 1, self.W + 1, dtype=torch.float64)
        for a in range(2):
            for c in range(2):
                y[a * 2 + c][:, :, :self.H + 1 - a, :self.W + 1 - c] = full[:, :, a::2, c::2]
        return y

    def _valid(self, y):
        return torch.cat([y[a * 2 + c][:, :, :self.H + 1 - a, :self.W + 1 - c].reshape(-1) for a in range(2) for c in range(2)])

    def defect(self, cus=None):
        t, p = self.tensors(), self.plan()
        ref = self._planes(t)
        if self.drop == 'reduce':
            bad = ref.clone()
            bad.view(-1)[p['reduce_grid'] * 1024:] = 0.0
        else:
            bad = self._planes(t, (p['ks'] - 1) * p['cps'] * p['KC'])
        return self._valid(ref), self._valid(bad), TOL_CONV

    def run(self, cus=None):
        kk = _kk()
        from shgan_amd import _lib
        t, p = self.tensors(), self.plan()
        ref = self._valid(self._planes(t))
        xd, pw = dev(t['x']), kk.conv_weight_prep(t['w'].to(DEV), gain=t['g'])
        if self.ws is None:
            call = lambda: self._valid(kk.conv2d(xd, pw, mode=kk.MODE_UP2T, planar=True))
        else:
            ws = torch.empty(max(p['ws_bytes'] // 4, 4), device=DEV)
            wa, wb = pw.up_poly()

            def call():
                y = torch.empty(4, 1, self.O, self.H + 1, self.W + 1, device=DEV)
                rc = _lib.get_lib().shg_conv2d_up_poly_ws_f32(_p(xd), _p(pw.wt), _p(wa), _p(wb), _p(y), 1, self.I, self.O, pw.op, self.H, self.W, None,
                                                              _p(ws), p['ws_bytes'], _stream())
                assert rc == 0, rc
                return self._valid(y)
        return call, ref, TOL_CONV, ('conv_poly_up_kernel', WSPLIT), (MFMA,), {}, {}


POLY_CASES = {
    # 33 chunks (I = 259) over 4 slices of 9, the last with 6 chunks of which the last holds 3 channels
    'poly_up_ragged_last_slice': PolyUp(259, 64, 16, 16, lambda p, c: p['nchunk'] % p['ks_fit'] != 0 and p['last'] < p['cps'] and 259 % c['POLY_KC'] != 0),
    'poly_up_workspace_half': PolyUp(512, 64, 16, 16, lambda p, c: p['halvings'] == 1 and p['ks'] == p['ks_planned'] // 2, ws=lambda full: full // 2),
    # 4 x 64 x 129 x 133 outputs: more float4 than one trip of wino_split_reduce_kernel's 4096 workgroups (113 workgroups, so the launch splits)
    'poly_up_reduce_second_trip': PolyUp(128, 64, 128, 132, lambda p, c: p['reduce_grid'] == c['WINO_REDUCE_CAP'] and p['out_bytes'] // 4 > p['reduce_grid'] * 1024
                                         and (p['out_bytes'] // 4) % (p['reduce_grid'] * 1024) != 0, drop='reduce'),
}


WINO_CASES = {
    # 33 chunks (I = 259: the last chunk holds 3 channels) over 4 slices of 9: the last slice has 6 chunks
    'wino_ragged_last_slice': Wino('wino', 259, 64, 16, 16, lambda p, c: _wsplit(True)(p, c) and 259 % c['WINO_KC'] != 0),
    'wino_workspace_half': Wino('wino', 512, 64, 16, 16, _wsplit(halved=1), ws=lambda full: full // 2),
    'wino_residual_8_not_16_unsplit': Wino('wino', 512, 64, 16, 16, lambda p, c: p['ks'] == 1 and p['ks_planned'] == 1 and
                                           P.wino_ksplit(p['tiles'], p['nchunk']) > 1, res='offset8', split=False),
    'wino4_ragged_last_slice': Wino('wino4', 259, 64, 32, 32, lambda p, c: _wsplit(True)(p, c) and 259 % c['WINO4_KC'] != 0),
    'wino4_workspace_half': Wino('wino4', 512, 64, 32, 32, _wsplit(halved=1), ws=lambda full: full // 2, res='aligned'),
    # 64 x 260 x 256 outputs: more float4 than wino_split_reduce_kernel's 4096 workgroups hold in one trip (reachable for the 512-pixel tiles of
    # F(4x4) only: test_plan_f32_cpu.py)
    'wino4_reduce_second_trip': Wino('wino4', 128, 64, 260, 256, lambda p, c: p['ks'] == 2 and P.wino_reduce_grid(1, 64, 260, 256) == c['WINO_REDUCE_CAP']
                                     and 64 * 260 * 256 > c['WINO_REDUCE_CAP'] * 1024 and (64 * 260 * 256) % (c['WINO_REDUCE_CAP'] * 1024) != 0, drop='reduce'),
}


# ------------------------------------------------------------------------------------------------
# FIR (upfirdn2d.hip, fir_march.h)
# ------------------------------------------------------------------------------------------------

def fir64(x, f, up=1, down=1, pad=(0, 0, 0, 0), flip=False, gain=1.0):
    """upfirdn2d of the planes x [NC, H, W] in float64: zero-insert, pad, correlate with the (flipped) filter, decimate -- sixteen shifted sums."""
    nc, h, w = x.shape
    z = torch.zeros(nc, h * up, w * up, dtype=torch.float64)
    z[:, ::up, ::up] = x.double()
    z = F.pad(z, list(pad))
    k = f.double() * gain
    if not flip:
        k = k.flip(0, 1)
    oh, ow = z.shape[1] - k.shape[0] + 1, z.shape[2] - k.shape[1] + 1
    y = torch.zeros(nc, oh, ow, dtype=torch.float64)
    for ky in range(k.shape[0]):
        for kx in range(k.shape[1]):
            y += k[ky, kx] * z[:, ky:ky + oh, kx:kx + ow]
    return y[:, ::down, ::down].contiguous()


def _sep():
    from oracle import shgan_oracle as orc
    return orc.setup_filter([1, 3, 3, 1])


class FirSame:
    """fir_same_kernel: each workgroup walks the planes nc, nc + gzs, ... with the next window prefetched."""

    def __init__(self, N, C, H, W, vec, epi=False, offset=0):
        self.N, self.C, self.H, self.W, self.vec, self.epi, self.offset = N, C, H, W, vec, epi, offset

    def plan(self):
        return P.fir_same_plan(self.N * self.C, self.H + 1, self.W + 1)

    def where(self, cus=None):
        p = self.plan()
        nc = self.N * self.C
        assert p['trips'] == 2 and nc > p['gzs'] and nc % p['gzs'] != 0 and p['last_trip'] < p['gzs'], p
        assert self.vec == (self.W % 4 == 0 and not self.offset)
        return p

    def tensors(self):
        n, c, oh, ow = self.N, self.C, self.H + 1, self.W + 1
        t = dict(x=rnd(121, n, c, self.H, self.W), f=rnd(122, 4, 4, lo=0.1))
        if self.epi:
            t.update(sc=rnd(123, n * c, lo=0.5), bi=rnd(124, c), nz=rnd(125, n, 1, oh, ow), res=rnd(126, n, c, oh, ow))
        return t

    def _finish(self, t, y):
        n, c = self.N, self.C
        y = y.view(n, c, *y.shape[1:])
        if self.epi:
            y = act64(y * t['sc'].double().view(n, c, 1, 1) + t['nz'].double() * 0.3 + t['bi'].double().view(1, c, 1, 1), True, gain=0.8) + t['res'].double()
        return y

    def defect(self, cus=None):
        """Second-trip planes computed from the first trip's window: plane nc >= gzs gets the FIR of plane nc - gzs."""
        t, p = self.tensors(), self.plan()
        y = fir64(t['x'].view(-1, self.H, self.W), t['f'], pad=(2, 2, 2, 2))
        bad = y.clone()
        bad[p['gzs']:] = y[:y.shape[0] - p['gzs']]
        return self._finish(t, y), self._finish(t, bad), TOL_PW

    def run(self, cus=None):
        kk = _kk()
        t = self.tensors()
        ref = self._finish(t, fir64(t['x'].view(-1, self.H, self.W), t['f'], pad=(2, 2, 2, 2)))
        xd, fd = dev(t['x'], self.offset), dev(t['f'])
        epi = None
        if self.epi:
            epi = dict(scale=dev(t['sc']), bias=dev(t['bi']), noise=dev(t['nz']), noise_strength=0.3, residual=dev(t['res']), act=True, gain=0.8)
        call = lambda: kk.upfirdn2d(xd, fd, padx0=2, padx1=2, pady0=2, pady1=2, epilogue=epi)
        name = 'fir_same_kernel<4, 4, true>' if self.vec else 'fir_same_kernel<4, 4, false>'
        other = 'fir_same_kernel<4, 4, false>' if self.vec else 'fir_same_kernel<4, 4, true>'
        return call, ref, TOL_PW, (name,), (other, 'fir_down_march_kernel', 'upfirdn_generic_kernel'), {name: 1}, {}


class FirDownPlanar:
    """fir_same_kernel in its planar-output form (shg_fir_down_planar_f32, the pre-filter of the polyphase stride-2 convolution): the grid covers
    the 2 PP x 2 PH2 extent of the four phase planes, every entry of which is written (zeros outside the filtered image)."""

    def __init__(self, NC, H, W, pp):
        self.NC, self.H, self.W, self.ph2, self.pp = NC, H, W, H // 2 + 1, pp
        assert pp % 4 == 0 and pp >= W // 2 + 1

    def plan(self):
        return P.fir_same_plan(self.NC, self.H + 1, self.W + 1, self.ph2, self.pp)

    def where(self, cus=None):
        p = self.plan()
        assert p['trips'] == 2 and self.NC % p['gzs'] != 0 and self.H % 2 == 0 and self.W % 2 == 0, p
        assert p['tiles'] != P.fir_same_plan(self.NC, self.H + 1, self.W + 1)['tiles'], 'the planar grid differs from the ordinary one'
        return p

    def tensors(self):
        return dict(x=rnd(181, self.NC, self.H, self.W), f=rnd(182, 4, 4, lo=0.1))

    def _planes(self, y):
        out = torch.zeros(4, self.NC, self.ph2, self.pp, dtype=torch.float64)
        for a in range(2):
            for b in range(2):
                q = y[:, a::2, b::2]
                out[a * 2 + b, :, :q.shape[1], :q.shape[2]] = q
        return out

    def defect(self, cus=None):
        t, p = self.tensors(), self.plan()
        y = fir64(t['x'], t['f'], pad=(2, 2, 2, 2))
        bad = y.clone()
        bad[p['gzs']:] = y[:y.shape[0] - p['gzs']]
        return self._planes(y), self._planes(bad), TOL_PW

    def run(self, cus=None):
        from shgan_amd import _lib
        t = self.tensors()
        ref = self._planes(fir64(t['x'], t['f'], pad=(2, 2, 2, 2)))
        xd, fd = dev(t['x']), dev(t['f'])

        def call():
            y = torch.empty(4, self.NC, self.ph2, self.pp, device=DEV)
            rc = _lib.get_lib().shg_fir_down_planar_f32(_p(xd), _p(fd), _p(y), 1, self.NC, self.H, self.W, self.pp, 0, 1.0, _stream())
            assert rc == 0, rc
            return y
        return call, ref, TOL_PW, ('fir_same_kernel<4, 4, true>',), ('fir_down_march_kernel',), {'fir_same_kernel': 1}, {}


class FirUpPlanar:
    """fir_up_planar_kernel (the generic form of upfir_planar) with the whole layer tail: the window of plane nc + gz is requested behind the
    noise rows (vector form) or straight after the barrier (scalar form)."""

    def __init__(self, N, C, H, W, vec):
        self.N, self.C, self.H, self.W, self.vec = N, C, H, W, vec

    def plan(self):
        return P.fir_up_planar_plan(self.N * self.C, self.H, self.W)

    def where(self, cus=None):
        p = self.plan()
        nc = self.N * self.C
        assert p['trips'] == 2 and nc > p['gz'] and nc % p['gz'] != 0, p
        assert self.vec == (self.W % 2 == 0)
        return p

    def tensors(self):
        n, c, h, w = self.N, self.C, self.H, self.W
        return dict(mid=rnd(131, 4, n, c, h + 1, w + 1), f=rnd(132, 4, 4, lo=0.1), sc=rnd(133, n * c, lo=0.5), bi=rnd(134, c),
                    nz=rnd(135, n, 1, 2 * h, 2 * w), res=rnd(136, n, c, 2 * h, 2 * w))

    def _fir(self, t):
        n, c, h, w = self.N, self.C, self.H, self.W
        full = torch.zeros(n * c, 2 * h + 1, 2 * w + 1, dtype=torch.float64)
        for a in range(2):
            for b in range(2):
                full[:, a::2, b::2] = t['mid'][a * 2 + b].reshape(n * c, h + 1, w + 1)[:, :h + 1 - a, :w + 1 - b].double()
        return fir64(full, t['f'], pad=(1, 1, 1, 1), gain=4.0)

    def _finish(self, t, y):
        n, c = self.N, self.C
        y = y.view(n, c, *y.shape[1:])
        return act64(y * t['sc'].double().view(n, c, 1, 1) + t['nz'].double() * 0.3 + t['bi'].double().view(1, c, 1, 1), True, gain=0.8) + t['res'].double()

    def defect(self, cus=None):
        t, p = self.tensors(), self.plan()
        y = self._fir(t)
        bad = y.clone()
        bad[p['gz']:] = y[:y.shape[0] - p['gz']]
        return self._finish(t, y), self._finish(t, bad), TOL_PW

    def run(self, cus=None):
        kk = _kk()
        t, p = self.tensors(), self.plan()
        ref = self._finish(t, self._fir(t))
        md, fd = dev(t['mid']), dev(t['f'])
        kw = dict(scale=dev(t['sc']), bias=dev(t['bi']), noise=dev(t['nz']), residual=dev(t['res']), noise_strength=0.3, act=True, gain=0.8)
        name = f'fir_up_planar_kernel<{"true" if self.vec else "false"}, {p["TV"]}>'
        return (lambda: kk.upfir_planar(md, fd, **kw)), ref, TOL_PW, (name,), ('fir_up_march_kernel',), {name: 1}, {}


class FirGeneric:
    """upfirdn_generic_kernel past its cap of planes in gridDim.z (tiny planes), and upfirdn_strided_kernel past its block cap."""

    def __init__(self, strided, N, C, H, W):
        self.strided, self.N, self.C, self.H, self.W = strided, N, C, H, W

    def plan(self):
        if self.strided:
            oh, ow = P.fir_out(self.H, self.W, 3, 5, 2, 1, (1, 2, 0, 1))
            return dict(P.fir_strided_plan(self.N * self.C * oh * ow), total=self.N * self.C * oh * ow)
        oh, ow = P.fir_out(self.H, self.W, 4, 4, 1, 2, (1, 1, 1, 1))
        return P.fir_generic_plan(self.N * self.C, oh, ow)

    def where(self, cus=None):
        p, c = self.plan(), P.constants()
        if self.strided:
            assert p['blocks'] == c['FIR_STRIDED_CAP'] and p['trips'] == 2 and p['total'] % (p['blocks'] * 256) != 0, p
        else:
            assert p['gz'] == c['FIR_GENERIC_GZ'] and p['trips'] == 2 and 0 < p['last_trip'] < p['gz'], p
        return p

    def tensors(self):
        if self.strided:
            return dict(x=rnd(141, self.N, self.C, self.W, self.H), f=rnd(142, 3, 5))          # stored [N, C, W, H]: read through exchanged strides
        return dict(x=rnd(141, self.N, self.C, self.H, self.W), f=rnd(142, 4, 4, lo=0.1))

    def _ref(self, t):
        if self.strided:
            return fir64(t['x'].transpose(2, 3).reshape(-1, self.H, self.W), t['f'], up=2, pad=(1, 2, 0, 1), gain=4.0)
        return fir64(t['x'].view(-1, self.H, self.W), t['f'], down=2, pad=(1, 1, 1, 1))

    def defect(self, cus=None):
        """Everything past the first trip of the grid left unwritten."""
        t, p = self.tensors(), self.plan()
        y = self._ref(t)
        bad = y.clone()
        if self.strided:
            bad.view(-1)[p['blocks'] * 256:] = 0.0
        else:
            bad[p['gz']:] = 0.0
        return y, bad, TOL_PW

    def run(self, cus=None):
        kk = _kk()
        t = self.tensors()
        ref = self._ref(t)
        fd = dev(t['f'])
        if self.strided:
            xd = t['x'].to(DEV).transpose(2, 3)
            call = lambda: kk.upfirdn2d_strided(xd, fd, 2, 2, 1, 1, 1, 2, 0, 1, False, 4.0).reshape(ref.shape)
            return call, ref, TOL_PW, ('upfirdn_strided_kernel<float, float>',), (), {}, {}
        xd = dev(t['x'])
        call = lambda: kk.upfirdn2d(xd, fd, downx=2, downy=2, padx0=1, padx1=1, pady0=1, pady1=1).reshape(ref.shape)
        return call, ref, TOL_PW, ('upfirdn_generic_kernel',), ('fir_dn2_march_kernel', 'fir_same_kernel'), {}, {}


class March:
    """The row-marching kernels: four items (waves) per workgroup, ``nitem % 4 != 0`` -- the last workgroup is partly idle."""

    def __init__(self, kind, kernel, N, C, H, W, wide=False):
        self.kind, self.kernel, self.N, self.C, self.H, self.W, self.wide = kind, kernel, N, C, H, W, wide

    def plan(self):
        return P.march_plan(self.kind, self.N * self.C, self.H, self.W, wide=self.wide)

    def where(self, cus=None):
        p = self.plan()
        assert p['nitem'] % 4 != 0 and p['grid'] >= 2 and p['grid'] * 4 > p['nitem'], p
        return p

    def tensors(self):
        n, c, h, w = self.N, self.C, self.H, self.W
        if self.kind == 'up':
            return dict(mid=rnd(151, 4, n, c, h + 1, w + 1), f=_sep(), sc=rnd(153, n * c, lo=0.5), bi=rnd(154, c), nz=rnd(155, n, 1, 2 * h, 2 * w),
                        res=rnd(156, n, c, 2 * h, 2 * w))
        t = dict(x=rnd(151, n, c, h, w), f=_sep())
        if self.wide:
            t.update(w=rnd(157, 8, c, 3, 3), b=rnd(158, 8))
        return t

    def _fir(self, t):
        """The FIR output as planes [NC, rows, cols] whose rows are the marched rows times ``rpr`` (output rows per marched row)."""
        h, w = self.H, self.W
        if self.kind == 'up':
            return FirUpPlanar._fir(self, t), 2
        x = t['x'].view(-1, h, w)
        if self.kind == 'down':
            return fir64(x, t['f'], pad=(2, 2, 2, 2)), 1
        if self.kind == 'dn2':
            return fir64(x, t['f'], down=2, pad=(1, 1, 1, 1)), 1
        return fir64(x, t['f'], up=2, pad=(2, 1, 2, 1), gain=4.0), 2

    def _finish(self, t, y):
        n, c = self.N, self.C
        if self.kind == 'up':
            return FirUpPlanar._finish(self, t, y)
        y = y.view(n, c, *y.shape[1:])
        if self.wide:                  # fir_conv_down2: the stride-2 3x3 convolution consumes the filtered planes
            return act64(F.conv2d(y, t['w'].double() / np.sqrt(c * 9), stride=2) + t['b'].double().view(1, -1, 1, 1), True)
        return y

    def defect(self, cus=None):
        """The items of the partly filled last workgroup dropped (a floor in place of cdiv(nitem, 4)): their rows stay unwritten."""
        t, p = self.tensors(), self.plan()
        y, rpr = self._fir(t)
        bad = y.clone()
        for item in range(p['nitem'] - p['nitem'] % 4, p['nitem']):
            seg, pg = item % p['nseg'], item // p['nseg']
            bad[pg * p['G']:(pg + 1) * p['G'], seg * p['R'] * rpr:(seg + 1) * p['R'] * rpr] = 0.0
        return self._finish(t, y), self._finish(t, bad), (TOL_CONV if self.wide else TOL_PW)

    def run(self, cus=None):
        kk = _kk()
        t = self.tensors()
        y, _ = self._fir(t)
        ref = self._finish(t, y)
        fd = dev(t['f'])
        if self.kind == 'up':
            md = dev(t['mid'])
            kw = dict(scale=dev(t['sc']), bias=dev(t['bi']), noise=dev(t['nz']), residual=dev(t['res']), noise_strength=0.3, act=True, gain=0.8)
            call = lambda: kk.upfir_planar(md, fd, **kw)
        elif self.wide:
            xd, bd = dev(t['x']), dev(t['b'])
            pw = kk.conv_weight_prep(t['w'].to(DEV), gain=1.0 / np.sqrt(self.C * 9))
            assert kk.down_poly_supported(xd, pw, force=True)
            call = lambda: kk.fir_conv_down2(xd, fd, pw, bias=bd, act=True)
        else:
            xd = dev(t['x'])
            up, dn, pad = {'down': (1, 1, (2, 2, 2, 2)), 'dn2': (1, 2, (1, 1, 1, 1)), 'up2': (2, 1, (2, 1, 2, 1))}[self.kind]
            call = lambda: kk.upfirdn2d(xd, fd, upx=up, upy=up, downx=dn, downy=dn, padx0=pad[0], padx1=pad[1], pady0=pad[2], pady1=pad[3],
                                        gain=4.0 if self.kind == 'up2' else 1.0)
        return call, ref, (TOL_CONV if self.wide else TOL_PW), (self.kernel,), ('fir_same_kernel', 'upfirdn_generic_kernel', 'fir_up_planar_kernel'), {}, {}


FIR_CASES = {
    'fir_same_vec_second_trip': FirSame(3, 683, 32, 64, True),                      # 4 tiles -> 2048 planes per trip, 2049 planes
    'fir_same_scalar_second_trip': FirSame(1, 4103, 32, 62, False),                 # W % 4 = 2; 2 tiles -> 4096 planes per trip
    'fir_same_vec_second_trip_layer_tail': FirSame(3, 683, 32, 64, True, epi=True),
    'fir_same_unaligned_second_trip_layer_tail': FirSame(3, 683, 32, 64, False, epi=True, offset=1),
    'fir_down_planar_second_trip': FirDownPlanar(2055, 32, 32, 36),                 # pitch 36: a 72 x 34 grid, 4 tiles (33 x 33 outputs: 2) -> 2048 planes per trip
    'fir_up_planar_vec_second_trip': FirUpPlanar(3, 1367, 17, 48, True),            # two 16 x 64 tiles -> 4096 planes per trip, 4101 planes
    'fir_up_planar_scalar_second_trip': FirUpPlanar(3, 1367, 17, 49, False),
    'fir_generic_past_plane_cap': FirGeneric(False, 5, 6555, 8, 8),                 # 32775 planes of 4 x 4 outputs
    'fir_strided_past_block_cap': FirGeneric(True, 2, 3, 700, 1000),
    'march_down_partial_workgroup': March('down', 'fir_down_march_kernel<1, 8, 0>', 1, 7, 40, 64),
    'march_down4_partial_workgroup': March('down', 'fir_down_march4_kernel<1, 8, 0>', 1, 7, 40, 256, wide=True),
    'march_up_partial_workgroup': March('up', 'fir_up_march_kernel<1, 2>', 1, 5, 24, 32),
    'march_dn2_partial_workgroup': March('dn2', 'fir_dn2_march_kernel<1>', 1, 5, 48, 64),
    'march_up2_partial_workgroup': March('up2', 'fir_up2_march_kernel<1>', 1, 5, 24, 64),
}


# ------------------------------------------------------------------------------------------------
# weight gradient (conv_wgrad.hip, conv_wgrad_wino.hip)
# ------------------------------------------------------------------------------------------------

class Wgrad:
    def __init__(self, kernel, N, I, O, H, W, edge, k=3, stride=1, pad=1, switches=None, offset=0):
        self.kernel, self.N, self.I, self.O, self.H, self.W, self.edge, self.k, self.stride, self.pad = kernel, N, I, O, H, W, edge, k, stride, pad
        self.switches, self.offset = dict(switches or {}), offset
        self.oh, self.ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        self.wino = kernel.startswith(WGW)

    def plan(self):
        if self.wino:
            return P.wgw_plan(self.N, self.I, self.O, self.H, self.W)
        return P.wgrad_chunks(self.N, self.I, self.O, self.H, self.W, self.oh, self.ow, self.k, self.stride, self.pad)

    def where(self, cus=None):
        p = self.plan()
        if not self.wino:
            assert p['kernel'].replace(' ', '') == self.kernel.replace(' ', ''), (p['kernel'], self.kernel)
        assert self.edge(p, P.constants()), f'{self.kernel} {self.N}x{self.I}->{self.O} {self.H}x{self.W}: no longer on its edge: {p}'
        return p

    def tensors(self):
        return dict(x=rnd(161, self.N, self.I, self.H, self.W), g=rnd(162, self.N, self.O, self.oh, self.ow))

    def chunk_ids(self, p):
        """The chunk that owns every gradient pixel, [N, OH, OW] (in the geometry of the call, not the flattened one)."""
        n, oh, ow = self.N, self.oh, self.ow
        nn, yy, xx = torch.meshgrid(torch.arange(n), torch.arange(oh), torch.arange(ow), indexing='ij')
        if self.wino:
            return (nn * p['cty'] + yy // p['rows']) * p['ctx'] + xx // p['cols']
        flat = (nn * oh + yy) * ow + xx
        if p['packed']:
            return flat // p['px']
        if p['two_rows']:
            return nn * (oh // 2) + yy // 2
        if p['full_rows']:
            return nn * (oh // p['full_rows']) + yy // p['full_rows']
        if p['OH'] == 1 and oh != 1:                # the flattened 1x1 form: an image is one row of H W pixels
            return nn * p['chunks_x'] + (yy * ow + xx) // p['px']
        return (nn * oh + yy) * p['chunks_x'] + xx // p['px']

    def _ref(self, t, g):
        return torch.nn.grad.conv2d_weight(t['x'].double(), (self.O, self.I, self.k, self.k), g, stride=self.stride, padding=self.pad)

    def defect(self, cus=None):
        """The last slice's chunks never added."""
        t, p = self.tensors(), self.plan()
        ids = self.chunk_ids(p)
        assert int(ids.max()) == p['nchunk'] - 1
        g = t['g'].double()
        keep = (ids < (p['used'] - 1) * p['per']).unsqueeze(1)
        return self._ref(t, g), self._ref(t, g * keep), TOL_CONV

    def run(self, cus=None):
        kk = _kk()
        t = self.tensors()
        ref = self._ref(t, t['g'].double())
        xd, gd = dev(t['x'], self.offset), dev(t['g'])
        others = [k for k in ('conv_wgrad_kernel', 'conv_wgrad_full_kernel', 'conv_wgrad_packed_kernel', WGW, 'wgrad_thin_kernel')
                  if not self.kernel.startswith(k)]
        return (lambda: kk.conv2d_wgrad(xd, gd, self.k, self.k, self.stride, self.pad)), ref, TOL_CONV, (self.kernel, 'wgrad_reduce_kernel'), others, {}, \
            self.switches


def _slices(by, several=True, ragged=True, per_image=None):
    """by: what limits the slice count -- 'target' (workgroup target / tiles), 'nchunk', 'cap' (1024); per_image: chunks per image, when a slice
    boundary is to fall inside an image."""
    def edge(p, c):
        ok = p['nslice'] > 1
        if several:
            ok = ok and p['per'] >= 2
        if ragged:
            ok = ok and 0 < p['last'] < p['per']
        if by == 'nchunk':
            ok = ok and p['nslice'] == p['nchunk'] and p['per'] == 1
        if by == 'cap':
            ok = ok and p['nslice'] == c['WGRAD_MAX_SLICES'] < p['nchunk']
        if per_image:
            ok = ok and p['nchunk'] % per_image == 0 and per_image % p['per'] != 0
        return ok
    return edge


NOWGW = {'WGRAD_WINO': False}

WGRAD_CASES = {
    # 256 -> 256 channels: 16 tiles, 16 slices; 2 x 33 rows of one 64-pixel chunk = 66 chunks: 5 per slice, 14 slices used, the last has 1; the
    # boundaries fall inside an image (33 chunks per image)
    'wgrad_rows_several_chunks_short_last': Wgrad('conv_wgrad_kernel<3, 3, 1, 1>', 2, 256, 256, 33, 50, _slices('target', per_image=33), switches=NOWGW),
    # 64 -> 64: one tile, 256 slices over 2 x 37 x 5 = 370 chunks (W = 290: five 64-pixel pieces per row): 2 per slice, boundaries inside rows
    'wgrad_slice_boundary_inside_row': Wgrad('conv_wgrad_kernel<3, 3, 1, 1>', 2, 64, 64, 37, 290, lambda p, c: _slices('target', ragged=False)(p, c)
                                             and p['chunks_x'] % p['per'] != 0 and p['chunks_x'] > 1, switches=NOWGW),
    'wgrad_slices_limited_by_nchunk': Wgrad('conv_wgrad_kernel<3, 3, 1, 1>', 1, 64, 64, 9, 50, _slices('nchunk', several=False, ragged=False), switches=NOWGW),
    'wgrad_full_s2_several_chunks': Wgrad('conv_wgrad_full_kernel<3, 3, 2, 1>', 2, 256, 256, 67, 65, _slices('target'), stride=2, pad=0),
    'wgrad_packed_several_chunks': Wgrad('conv_wgrad_packed_kernel<3, 3, 1>', 10, 256, 256, 16, 16, _slices('target'), switches=NOWGW),
    # 1x1: the target is 1024 workgroups; 2 x 2 tiles: 256 slices over 7 x 47 chunks of 64 pixels: 2 per slice, the last has 1
    'wgrad_1x1_target_1024': Wgrad('conv_wgrad_full_kernel<1, 1, 1, 1>', 7, 128, 128, 47, 64, lambda p, c: _slices('target')(p, c)
                                   and p['nslice'] == c['WGRAD_WG_1X1'] // 4, k=1, pad=0),
    'wgrad_1x1_slices_at_cap_1024': Wgrad('conv_wgrad_full_kernel<1, 1, 1, 1>', 2, 64, 64, 130, 256, _slices('cap', ragged=False), k=1, pad=0),
    'wgrad_wino_several_chunks_short_last': Wgrad(f'{WGW}<3>', 3, 256, 256, 20, 36, _slices('target')),
}


CASES = {}
for _tab in (CONV_CASES, POLY_CASES, WINO_CASES, FIR_CASES, WGRAD_CASES):
    assert not set(_tab) & set(CASES)
    CASES.update(_tab)


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(CASES))
def test_loop_bound(case):
    kk = _kk()
    cus = _cus()
    obj = CASES[case]
    obj.where(cus)
    call, ref, tol, expect, forbid, counts, switches = obj.run(cus)
    old = {k: getattr(kk, k) for k in switches}
    try:
        for k, v in switches.items():
            setattr(kk, k, v)
        got, launches = launch_counts(call, expect=expect, want=counts)
    finally:
        for k, v in old.items():
            setattr(kk, k, v)
    kern = sorted(n for n in launches if 'kernel' in n)
    for p in expect:
        assert any_hit(p, launches), f'{case}: expected {p} to run; ran {kern}'
    for p in forbid:
        assert not any_hit(p, launches), f'{case}: {p} must not run; ran {kern}'
    for p, want in counts.items():
        have = count_of(p, launches)
        assert have == want, f'{case}: {p} launched {have} times, the plan says {want}; ran {kern}'
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.reshape(-1)
    assert got.shape == ref.shape, (case, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), case
    e = rel_err(got.numpy(), ref.numpy())
    print(f'LOOP {case} rel_err={e:.3e} (tol {tol:.0e}, {ref.numel()} values compared)')
    assert e < tol, f'{case}: rel err {e:.3e} >= {tol:.0e}'


# ------------------------------------------------------------------------------------------------
# optimiser (optim.hip): chunks past OPT_MAX_BLOCKS
# ------------------------------------------------------------------------------------------------

def opt_shapes():
    """A parameter set of more than OPT_MAX_BLOCKS chunks: one tensor that starts before the cap and ends behind it, with small ones on both
    sides -- whichever way the gradient buckets are packed (in this order or reversed), the large one sits at an odd float offset and a small
    one lies wholly behind the cap; the GPU tests assert both from the tables they launch with.  The last parameter never receives a gradient."""
    c = P.constants()
    assert c['OPT_CHUNK'] == 4096
    return [(3,), (2049 * 4096 + 5,), (7, 9), (1025,), (5,), (34,)]          # (fixed sizes: a raised OPT_MAX_BLOCKS takes the cases off their edge)


def opt_plan(shapes=None):
    c = P.constants()
    shapes = opt_shapes() if shapes is None else shapes
    first = np.concatenate([[0], np.cumsum([P.cdiv(int(np.prod(s)), c['OPT_CHUNK']) for s in shapes])])
    return dict(first=first, chunks=int(first[-1]), **P.opt_grid(int(first[-1])))


def opt_unstepped(shapes=None):
    """Per tensor: the first element that only a chunk >= OPT_MAX_BLOCKS (a second trip of the grid) updates (None: the whole tensor is first-trip).
    A segment's up to three elements before its first 16-byte boundary belong to its chunk 0, hence the margin of 4."""
    c, p = P.constants(), opt_plan(shapes)
    shapes = opt_shapes() if shapes is None else shapes
    out = []
    for i, s in enumerate(shapes):
        n = int(np.prod(s))
        k = (c['OPT_MAX_BLOCKS'] - int(p['first'][i])) * c['OPT_CHUNK']
        out.append(None if k >= n else max(k + 4, 0) if k > 0 else 0)
    return out


def _adam_big(steps=2, seed=0):
    import shgan_amd  # noqa: F401
    import adam_f64
    from shgan_amd import optim
    from shgan_amd.grad_sync import BucketedAllReduce
    from test_gpu_optim import bits, special_grad
    shapes = opt_shapes()
    rs = np.random.RandomState(seed)
    init = [rs.standard_normal(s).astype(np.float32) for s in shapes]
    params = [torch.nn.Parameter(torch.from_numpy(a).to(DEV)) for a in init]
    ref_params = [torch.nn.Parameter(torch.from_numpy(a).to(DEV)) for a in init]
    sync = BucketedAllReduce(params, bucket_bytes=1 << 28)
    big = max(range(len(shapes)), key=lambda i: int(np.prod(shapes[i])))
    assert len(sync.buckets) == 1 and sync.slot(params[big])[1] % 2 == 1, 'the large tensor sits at an odd float offset of its bucket'
    lr, betas, eps = 0.002, (0.9, 0.999), 1e-8
    opt = optim.ShgAdam(params, lr=lr, betas=betas, eps=eps, sync=sync)
    tab, cap = opt.host_table(None), P.constants()['OPT_MAX_BLOCKS']
    order = sorted(range(len(shapes)), key=lambda i: sync.slot(params[i])[1])                   # the streaming order: ascending bucket offsets
    assert [int(r[4]) for r in tab[:-1]] == [int(np.prod(shapes[i])) for i in order]
    assert [int(v) for v in tab[:, -1]] == [int(v) for v in opt_plan([shapes[i] for i in order])['first']] and int(tab[-1, -1]) > cap
    row = order.index(big)
    assert int(tab[row, -1]) < cap < int(tab[row + 1, -1]) and int(tab[-2, -1]) >= cap, 'the large tensor crosses the cap, a small one lies behind it'
    ref = torch.optim.Adam(ref_params, lr=lr, betas=betas, eps=eps, foreach=True, fused=False)
    y = [dict(p=a.astype(np.float64), m=np.zeros(a.shape), v=np.zeros(a.shape), t=0) for a in init]
    touched = list(range(len(params) - 1))
    for step in range(steps):
        grads = {i: special_grad(shapes[i], rs) for i in touched}
        sync.zero_grad()
        with torch.enable_grad():
            sum((params[i] * torch.from_numpy(grads[i]).to(DEV)).sum() for i in touched).backward()
        g_in = {i: params[i].grad.detach().clone() for i in touched}
        before = [b.clone() for b in sync.buckets]
        last = params[-1]
        keep = [t.clone() for t in (last, opt.state[last]['exp_avg'], opt.state[last]['exp_avg_sq'], opt.state[last]['step'])]
        opt.step_from_buckets(world=1)
        for b0, b1 in zip(before, sync.buckets):                 # exact: the gradient write-back (sanitised in place)
            assert torch.equal(bits(torch.nan_to_num(b0, nan=0.0, posinf=1e5, neginf=-1e5)), bits(b1)), 'gradient write-back differs'
        st = opt.state[last]                                     # exact: the untouched parameter and its state
        assert last.grad is None and torch.equal(bits(keep[0]), bits(last)) and torch.equal(bits(keep[1]), bits(st['exp_avg']))
        assert torch.equal(bits(keep[2]), bits(st['exp_avg_sq'])) and float(keep[3]) == float(st['step']) == 0.0
        for i in range(len(params)):
            ref_params[i].grad = None
        for i in touched:
            ref_params[i].grad = torch.nan_to_num(g_in[i].clone(), nan=0.0, posinf=1e5, neginf=-1e5)
            g64 = adam_f64.sanitize_f64(g_in[i].cpu().numpy(), 1)
            y[i]['p'], y[i]['m'], y[i]['v'], y[i]['t'] = adam_f64.adam_step_f64(y[i]['p'], g64, y[i]['m'], y[i]['v'], y[i]['t'], lr, betas[0], betas[1], eps)
        ref.step()
    torch.cuda.synchronize()
    return params, opt, ref_params, ref, y, touched


@pytest.mark.gpu
def test_adam_chunks_past_the_grid_cap():
    """Two steps over opt_shapes(): 2052 chunks on a grid capped at OPT_MAX_BLOCKS = 2048 workgroups, so the end of the large tensor (at an odd
    float offset of its bucket) and all of the tensors behind it are updated in a second trip of the grid-stride loop.  Gradients hold NaN, the
    infinities, denormals and zeros; the last parameter never gets one.  Exact (inside ``_adam_big``): the sanitised gradient written back,
    the untouched parameter and its state.  p, exp_avg, exp_avg_sq: the 2 x rule of tests/test_gpu_optim.py against the float64 yardstick."""
    import adam_f64
    params, opt, ref_params, ref, y, touched = _adam_big()
    for key, name in (('p', None), ('m', 'exp_avg'), ('v', 'exp_avg_sq')):
        eo = et = 0.0
        for i in touched:
            p = params[i]
            a = (p if name is None else opt.state[p][name]).detach().cpu().numpy()
            b = (ref_params[i] if name is None else ref.state[ref_params[i]][name]).detach().cpu().numpy()
            assert np.isfinite(a).all()
            eo, et = max(eo, adam_f64.rel_err(a, y[i][key])), max(et, adam_f64.rel_err(b, y[i][key]))
            assert float(opt.state[p]['step']) == y[i]['t'] == 2.0
        print(f'Adam past the cap {key}: ShgAdam {eo:.3e}, torch float32 {et:.3e} (vs float64 yardstick)')
        assert eo <= 2 * et, (key, eo, et)


class _BigNet(torch.nn.Module):
    """Parameters (lerp segments) and buffers (copy segments) of opt_shapes(): the large parameter crosses the cap, the buffers lie behind it."""

    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s, generator=g)) for s in opt_shapes()[:3]])
        self.register_buffer('f', torch.randn(3 * 4096 + 29, generator=g))
        self.register_buffer('i64', torch.randint(-2 ** 62, 2 ** 62, (5,), generator=g, dtype=torch.int64))


@pytest.mark.gpu
def test_ema_chunks_past_the_grid_cap():
    """EmaUpdater over the same sizes: the lerp segment of the large parameter crosses chunk OPT_MAX_BLOCKS, a lerp segment and two copy segments
    (one of four chunks) lie wholly behind it.  Two updates with G moving in between; p_ema under the 2 x rule against the float64 lerp, the
    buffers bit for bit."""
    import shgan_amd  # noqa: F401
    import adam_f64
    from shgan_amd import optim, train_stage as ts
    G, G_ema, G_ref = _BigNet(1).to(DEV), _BigNet(2).to(DEV), _BigNet(2).to(DEV)
    y = [p.detach().cpu().numpy().astype(np.float64) for p in G_ema.parameters()]
    ema = optim.EmaUpdater(G_ema, G)
    tab, cap = ema.host_table, P.constants()['OPT_MAX_BLOCKS']
    kinds = [(int(r[3]), int(r[5])) for r in tab[:-1]]
    assert int(tab[-1, -1]) > cap and any(k == optim.EMA_LERP and c0 >= cap for k, c0 in kinds) and any(k == optim.EMA_COPY and c0 >= cap for k, c0 in kinds)
    assert any(k == optim.EMA_LERP and c0 < cap < int(tab[i + 1, 5]) for i, (k, c0) in enumerate(kinds))
    for cur_nimg in (640, 6400):
        beta = ema.update(32, cur_nimg, ema_kimg=10.0, ema_rampup=0.05)
        assert beta == ts.update_ema(G_ref, G, 32, cur_nimg, 10.0, 0.05)
        b32 = float(np.float32(beta))
        for i, p in enumerate(G.parameters()):
            y[i] = adam_f64.ema_f64(y[i], p.detach().cpu().numpy(), b32)
        for (n, b), (_, b_ema) in zip(G.named_buffers(), G_ema.named_buffers()):
            assert torch.equal(b.view(torch.int32) if b.element_size() == 4 else b, b_ema.view(torch.int32) if b.element_size() == 4 else b_ema), n
        with torch.no_grad():
            for p in G.parameters():
                p.mul_(1.01).add_(0.003)
            G.f.mul_(1.5)
            G.i64.add_(7)
    eo = max(adam_f64.rel_err(p.detach().cpu().numpy(), y[i]) for i, p in enumerate(G_ema.parameters()))
    et = max(adam_f64.rel_err(p.detach().cpu().numpy(), y[i]) for i, p in enumerate(G_ref.parameters()))
    print(f'EMA past the cap: EmaUpdater {eo:.3e}, torch float32 lerp {et:.3e} (vs float64 yardstick)')
    assert eo <= 2 * et, (eo, et)
