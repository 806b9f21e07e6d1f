"""``inpaint.paste_back_membrane`` (csrc/membrane.hip) timed with device events after a warm-up, on the workload of tools/inpaint_bench.py:
8 photographs of 3000 x 2000 with a hole box of about 900 x 700 each (window 1800 x 1800), R = 512, feather = 16, K = 1 and K = 4.

Per K: the three stages (setup, solve, paste) timed apart, each between its own pair of events, several rounds in one process; the
solver's info (cycles, state, the residual norm where it stopped); the whole python call beside ``paste_back`` (the feather alone).
Once: the residual norm after every cycle (the per-cycle convergence factor) on the first problem of the workload and on a corridor
domain of the same size; the distance of the device's membrane from a float64 conjugate-gradient solve on the host (one problem, one
channel); the same solve composed from torch operators (float32 masked red-black relaxation, the same stop rule, capped).
The cycle's traffic on the fine level -- two smoother launches (13 bytes read, 12 written per pixel of a tile that holds Omega), the
restriction (13 read), the prolongation (13 read, 12 written) and the norm (13 read), 86 bytes per such pixel, the coarse levels a
third more -- over the time of a cycle stands beside the 6.0 / 6.3 TB/s of an in-order HBM sweep; the smoother alone is not isolated
(the entry point enqueues the whole sequence).  Prints one JSON line per measurement; ``--out`` also writes them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import shgan_amd  # noqa: E402,F401
from shgan_amd import inpaint, resize  # noqa: E402

DEV = 'cuda:0'
SWEEP_TBS = (6.0, 6.3)


def norm_of(info_row):
    return float(np.array([info_row[1]], np.int32).view(np.float32)[0])


def stats(xs):
    xs = sorted(xs)
    return {'us_median': round(xs[len(xs) // 2], 1), 'us_min': round(xs[0], 1), 'us_max': round(xs[-1], 1), 'rounds': len(xs)}


def cycle_norms(field, omega, h, w, n, cycles):
    """The residual norm before the first cycle and after every cycle: one-cycle solves on the same field (a cycle starts its coarse
    levels from 0, so this is the arithmetic of one long solve)."""
    norms = [norm_of(inpaint.membrane_solve(field, omega, np.array([[h, w, 0, 0]]), tol=1e-30, max_cycles=0, n=np.array([n])).cpu().numpy()[0])]
    for _ in range(cycles):
        info = inpaint.membrane_solve(field, omega, np.array([[h, w, 0, 0]]), tol=1e-30, max_cycles=1, n=np.array([n])).cpu().numpy()[0]
        norms.append(norm_of(info))
        if info[2] == 2:
            break
    return norms


def torch_relax(f, om, res_tol, cap, check=100):
    """float32 masked red-black Gauss-Seidel from torch operators: f [h, w, 3] (Dirichlet data outside om, 0 inside), om bool [h, w]."""
    h, w = om.shape
    yy, xx = torch.meshgrid(torch.arange(h, device=f.device), torch.arange(w, device=f.device), indexing='ij')
    colour = [(om & (((yy + xx) & 1) == p))[:, :, None] for p in (0, 1)]
    u = f.clone()

    def nbsum(u):
        p = F.pad(u.permute(2, 0, 1), (1, 1, 1, 1)).permute(1, 2, 0)
        return p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:]
    sweeps, norm = 0, float('inf')
    while sweeps < cap:
        for _ in range(check):
            for c in colour:
                u = torch.where(c, 0.25 * nbsum(u), u)
        sweeps += check
        norm = float(((4 * u - nbsum(u)).abs() * om[:, :, None]).max())
        if norm <= res_tol:
            break
    return u, sweeps, norm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--height', type=int, default=2000)
    ap.add_argument('--width', type=int, default=3000)
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--feather', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--torch-cap', type=int, default=2000)
    ap.add_argument('--no-host-solve', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('membrane_bench needs a GPU')
    import membrane_f64 as mref
    B, H, W, R, feather = a.images, a.height, a.width, a.resolution, a.feather
    rs = np.random.RandomState(0)
    imgs = [rs.randint(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(B)]
    masks, boxes = [], []
    for _ in range(B):
        bh, bw = int(0.35 * H + rs.randint(-20, 21)), int(0.30 * W + rs.randint(-20, 21))
        ya, xa = int(rs.randint(0, H - bh)), int(rs.randint(0, W - bw))
        m = np.ones((H, W), np.uint8)
        m[ya:ya + bh, xa:xa + bw] = 0
        masks.append(m)
        boxes.append((ya, ya + bh, xa, xa + bw))
    boxes = np.array(boxes)
    windows = np.array([inpaint.plan_window(m, R, 0.5, feather) for m in masks], np.int64)
    packed, shapes = resize.pack_images(imgs)
    pm, moffs = inpaint.pack_masks(masks)
    shapes = np.concatenate([shapes.numpy().astype(np.int64), moffs[:, None]], axis=1)
    packed, pm = packed.to(DEV), pm.to(DEV)
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    ev = lambda: torch.cuda.Event(enable_timing=True)                 # noqa: E731
    first = None
    for k in (1, 4):
        fake = (torch.rand(B * k, 3, R, R, device=DEV) * 1.6 - 0.8)
        plan = inpaint.membrane_plan(shapes, windows, feather, k, boxes)
        g = torch.empty(plan.g_elems, device=DEV)
        field = torch.empty(plan.g_elems, device=DEV)
        omega = torch.empty(plan.omega_bytes, dtype=torch.uint8, device=DEV)
        ws = torch.empty(plan.ws_bytes, dtype=torch.uint8, device=DEV)
        info = torch.empty(B * k, 3, dtype=torch.int32, device=DEV)
        out = packed.repeat(k).view(k, -1)
        times = {'setup': [], 'solve': [], 'paste': [], 'paste_back_membrane (python call)': [], 'paste_back (python call)': []}
        for rnd in range(a.rounds + 1):                               # round 0 warms up
            e = [ev() for _ in range(6)]
            e[0].record()
            inpaint.membrane_setup(packed, pm, shapes, windows, fake, plan, g, field, omega, feather)
            e[1].record()
            inpaint.membrane_solve(field, omega, plan.table, 0.25, None, info, None, plan.n, ws)
            e[2].record()
            inpaint.membrane_paste(pm, shapes, windows, plan, g, field, out, R, feather)
            e[3].record()
            inpaint.paste_back_membrane(packed, pm, shapes, windows, fake, k=k, feather=feather, out=out, boxes=boxes)
            e[4].record()
            inpaint.paste_back(packed, pm, shapes, windows, fake, k=k, feather=feather, out=out)
            e[5].record()
            torch.cuda.synchronize()
            if rnd:
                for name, i in zip(times, range(5)):
                    times[name].append(e[i].elapsed_time(e[i + 1]) * 1e3)
        inf = info.cpu().numpy()
        om_px = int(sum(int(omega[o:o + h * w].count_nonzero()) for (_, _, h, w, _, o) in plan.grids.tolist()))
        grid_px = int((plan.grids[:, 2] * plan.grids[:, 3]).sum())
        for name, xs in times.items():
            emit(dict(what=name, K=k, problems=B * k, grid_px_per_sample=grid_px, omega_px_per_sample=om_px, **stats(xs)))
        cyc = inf[:, 0].astype(int)
        rec = dict(what='solver info', K=k, cycles=cyc.tolist(), states=inf[:, 2].tolist(), norms=[float(f'{norm_of(r):.3e}') for r in inf],
                   res_tol=[float(f'{8 * 0.25 / (n + 1) ** 2:.3e}') for n in plan.n.tolist()], g_field_omega_bytes=8 * plan.g_elems + plan.omega_bytes,
                   workspace_bytes=plan.ws_bytes)
        solve_us = stats(times['solve'])['us_median']
        per_cycle = solve_us / max(float(cyc.max()), 1.0)
        moved = 86.0 * 4 / 3 * om_px * k                              # (Omega's tiles hold a little more than Omega: a lower bound)
        rec.update(us_per_cycle=round(per_cycle, 1), bytes_per_cycle=int(moved), TB_per_s=round(moved / per_cycle * 1e-6, 3),
                   of_sweep=[round(moved / per_cycle * 1e-6 / s, 3) for s in SWEEP_TBS])
        emit(rec)
        if first is None:
            gy0, gx0, gh, gw, foff, ooff = plan.grids[0].tolist()
            inpaint.membrane_setup(packed, pm, shapes, windows, fake, plan, g, field, omega, feather)
            first = (field[foff:foff + 3 * gh * gw].clone(), omega[ooff:ooff + gh * gw].clone(), gh, gw, int(plan.n[0]))

    # convergence per cycle, the float64 distance and the torch composition, on the first problem
    f0, om0, gh, gw, n = first
    res_tol = 8 * 0.25 / (n + 1) ** 2
    work = f0.clone()
    norms = cycle_norms(work, om0, gh, gw, n, 30)
    emit(dict(what='norm after each cycle, bench shape', h=gh, w=gw, n=n, res_tol=float(f'{res_tol:.3e}'), norms=[float(f'{x:.3e}') for x in norms],
              factors=[round(b / a_, 3) for a_, b in zip(norms, norms[1:]) if a_ > 0]))
    side = 900
    cor = mref.domain('corridor', side, side)
    fc = torch.from_numpy(mref.random_field(cor, 1).reshape(-1)).to(DEV)
    norms = cycle_norms(fc, torch.from_numpy(cor.astype(np.uint8).reshape(-1)).to(DEV), side, side, mref.omega_box_side(cor), 30)
    emit(dict(what='norm after each cycle, corridor shape', h=side, w=side, norms=[float(f'{x:.3e}') for x in norms],
              factors=[round(b / a_, 3) for a_, b in zip(norms, norms[1:]) if a_ > 0]))
    work = f0.clone()
    info = inpaint.membrane_solve(work, om0, np.array([[gh, gw, 0, 0]]), n=np.array([n])).cpu().numpy()[0]
    dev_c = work.cpu().numpy().reshape(gh, gw, 3)
    om_h = om0.cpu().numpy().reshape(gh, gw) != 0
    t0 = time.time()
    u, sweeps, tnorm = torch_relax(f0.view(gh, gw, 3), om0.view(gh, gw) != 0, res_tol, a.torch_cap)
    torch.cuda.synchronize()
    t_torch = time.time() - t0
    emit(dict(what='torch red-black relaxation, one problem', sweeps=sweeps, cap=a.torch_cap, seconds=round(t_torch, 3), norm_reached=float(f'{tnorm:.3e}'),
              res_tol=float(f'{res_tol:.3e}'), reached=bool(tnorm <= res_tol)))
    if not a.no_host_solve:
        t0 = time.time()
        c64 = mref.solve_reference(f0.cpu().numpy().reshape(gh, gw, 3)[:, :, 0], om_h, rtol=1e-8)
        emit(dict(what='distance to the float64 solve, one problem, channel 0', state=int(info[2]), cycles=int(info[0]), norm=float(f'{norm_of(info):.3e}'),
                  max_abs_c_minus_c64=float(f'{np.abs(dev_c[:, :, 0] - c64).max():.3e}'), max_abs_data=float(np.abs(c64[~om_h]).max()),
                  torch_max_abs_c_minus_c64=float(f'{np.abs(u[:, :, 0].cpu().numpy() - c64).max():.3e}'), host_seconds=round(time.time() - t0, 1)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            for r in records:
                fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
