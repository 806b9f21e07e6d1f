"""The launch plans of the float32 convolution, FIR, weight-gradient and optimiser kernels, restated on the host (no GPU, no library call).

Each function returns, for given shapes, what the launch code of ``sh-gan_amd/csrc`` decides: tile shapes, K-split factors, grid sizes, trips
per workgroup.  Every number the decisions hang on (grid caps, fill targets, minimum chunks per slice, chunk sizes, the tail-split rule) is READ
from the .hip / .h sources by ``constants()`` -- a changed constant moves the plan, and the cases of tests/test_gpu_loop_bounds_fp32.py assert
from the plan that they still sit on their edge (tests/test_plan_f32_cpu.py).  The scan patterns quote the source lines they read: a rewritten
line makes the scan fail with the pattern's name instead of silently keeping an old value.  Nothing here is shipped."""
import functools
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sh-gan_amd', 'csrc')


def cdiv(a, b):
    return -(-a // b)


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _scan(text, pattern, what):
    m = re.search(pattern, text)
    assert m, f'launch-plan scan: the source line of "{what}" changed (pattern {pattern!r})'
    return [int(g) for g in m.groups()]


@functools.lru_cache(maxsize=None)
def constants():
    """name -> int, scanned from the sources (see the module docstring)."""
    c = {}
    s = _src('conv_mfma.hip')
    c['KS_FILL'], c['KS_MIN_CHUNKS'], c['KS_MAX'] = _scan(
        s, r'while \(grid \* ks < (\d+) && chunks / \(ks \* 2\) >= (\d+) && ks < (\d+)\) ks \*= 2;', 'conv_ksplit')
    c['TAIL_NUM'], c['TAIL_DEN'] = _scan(s, r'nwork > slots && tail > 0 && tail \* (\d+) < slots \* (\d+)', 'tail split: the 60 % rule')
    c['TAIL_KS_MAX'], c['TAIL_MIN_CHUNKS'] = _scan(
        s, r'while \(tk < (\d+) && tail \* tk \* 2 <= slots && chunks / \(tk \* 2\) >= (\d+)\) tk \*= 2;', 'tail split: slices per tail tile')
    a, b = _scan(s, r'int rg = shg_cdiv\(out_elems, 256\); if \(rg > (\d+)\) rg = (\d+);', 'splitk_reduce grid cap')
    assert a == b
    c['SPLITK_REDUCE_CAP'] = a
    c['TW_MIN'], b = _scan(s, r'if \(tw < (\d+) && tw != cols && cols >= (\d+)\) continue;', 'tile_search: short rows')
    assert c['TW_MIN'] == b
    c['TW_FALLBACK'], b = _scan(s, r'if \(best < 0\) \{ btw = cols < (\d+) \? cols : (\d+); bth = 1; btn = 1; \}', 'tile_search: nothing fits')
    assert c['TW_FALLBACK'] == b
    c['TW_FULL'], = _scan(s, r'const int full = \(tw % (\d+) == 0\) \? 1 : 0;', 'tile_search: full store segments')
    v = _scan(s, r'return \(size_t\)(\d+) \* \(up \? (\d+) \* (\d+) \* (\d+) : (\d+) \* (\d+)\) \* sizeof\(float\);', 'conv_tail_ws_bound')
    c['TAIL_WS_UP'], c['TAIL_WS'] = v[0] * v[1] * v[2] * v[3] * 4, v[0] * v[4] * v[5] * 4
    c['CONV_UP_MIN'], = _scan(s, r'static constexpr int CONV_UP_MIN = (\d+);', 'CONV_UP_MIN')
    c['CU_DEFAULT'], = _scan(_src('shg_common.h'), r'\|\| c <= 0\) c = (\d+);', 'shg_cu_count default')
    s = _src('conv_wino.hip')
    c['WINO_KC'], = _scan(s, r'namespace wino \{[^}]*?constexpr int KC = (\d+),', 'wino::KC')
    c['WINO_FILL'], c['WINO_MIN_CHUNKS'] = _scan(s, r'while \(tiles \* ks < (\d+) && nchunk / \(ks \* 2\) >= (\d+)\) ks \*= 2;', 'shg_wino_ksplit')
    a, b = _scan(s, r'if \(grid > (\d+)\) grid = (\d+);', 'wino_split_reduce grid cap')
    assert a == b
    c['WINO_REDUCE_CAP'] = a
    v = _scan(s, r'const bool wide = W >= (\d+); .*\n\s*p\.tiles_x = shg_cdiv\(W, wide \? (\d+) : (\d+)\); p\.tiles_y = shg_cdiv\(H, wide \? (\d+) : (\d+)\);',
              'wino_plan')
    c['WINO_WIDE_W'], c['WINO_TW_WIDE'], c['WINO_TW'], c['WINO_TH_WIDE'], c['WINO_TH'] = v
    c['WINO_MAX_CHUNKS'], = _scan(s, r'SHG_CHECK_ARG\(I <= (\d+) \* wino::KC,', 'conv2d_wino: channel limit')
    s = _src('conv_wino4.hip')
    c['WINO4_KC'], = _scan(s, r'namespace wino4 \{[^}]*?constexpr int KC = (\d+),', 'wino4::KC')
    c['URING_WIDE_MIN_I'], = _scan(s, r'constexpr int URING_WIDE_MIN_I = (\d+);', 'wino4::URING_WIDE_MIN_I')
    v = _scan(s, r'const int shape = \(W >= (\d+) && H >= (\d+) && !\(narrow && H >= (\d+)\)\) \? 2 : \(\(W >= (\d+) && H >= (\d+)\) \? 1 : 0\);\n'
                 r'\s*p\.tiles_x = shg_cdiv\(W, (\d+) << shape\); p\.tiles_y = shg_cdiv\(H, (\d+) >> shape\);', 'wino4_plan')
    c['W4_S2_W'], c['W4_S2_H'], c['W4_S2_NARROW_H'], c['W4_S1_W'], c['W4_S1_H'], c['W4_TW'], c['W4_TH'] = v
    s = _src('conv_wino_poly.hip')
    c['POLY_KC'], = _scan(s, r'namespace poly \{[^}]*?constexpr int KC = (\d+),', 'poly::KC')
    s = _src('upfirdn2d.hip')
    a, b = _scan(s, r'const int gz = p\.NC < (\d+) \? p\.NC : (\d+);', 'upfirdn_generic plane cap')
    assert a == b
    c['FIR_GENERIC_GZ'] = a
    c['FIR_SAME_WG'], = _scan(s, r'int gzs = (\d+) / tiles; if \(gzs < 1\) gzs = 1; if \(gzs > p\.NC\) gzs = p\.NC;', 'fir_same: workgroup target')
    c['FIR_SAME_TW'], c['FIR_SAME_TH'] = _scan(s, r'const int tiles = shg_cdiv\(cov_w, (\d+)\) \* shg_cdiv\(cov_h, (\d+)\);', 'fir_same: tile')
    c['FIR_GENERIC_TW'], c['FIR_GENERIC_TH'] = _scan(s, r'dim3 grid\(shg_cdiv\(p\.OW, (\d+)\), shg_cdiv\(p\.OH, (\d+)\), gz\);', 'upfirdn_generic: tile')
    a, b = _scan(s, r'if \(blocks > (\d+)\) blocks = (\d+);', 'upfirdn_strided block cap')
    assert a == b
    c['FIR_STRIDED_CAP'] = a
    c['FIR_UP_WG'], = _scan(s, r'int gz = (\d+) / tiles; if \(gz < 1\) gz = 1; if \(gz > p\.NC\) gz = p\.NC;', 'fir_up_planar: workgroup target')
    v = _scan(s, r'const int TV = W >= (\d+) \? (\d+) : \(W >= (\d+) \? (\d+) : (\d+)\), TU = (\d+) / TV;', 'fir_up_planar: tile')
    c['FIR_UP_TV'] = tuple(v)
    m = re.findall(r'int nseg = shg_cdiv\((\d+), npg\);', s)
    assert len(m) == 3 and len(set(m)) == 1, 'marching kernels: wave target'
    c['MARCH_WAVES'] = int(m[0])
    c['MARCH_ROWS_DOWN'], = _scan(s, r'if \(nseg > OH / (\d+)\) nseg = OH / \d+;', 'fir_pad2_sep: rows per segment')
    c['MARCH_ROWS_UP'], = _scan(s, r'if \(nseg > H / (\d+)\) nseg = H / \d+;', 'upfir_planar_sep: rows per segment')
    c['MARCH_ROWS_RS'], = _scan(s, r'if \(nseg > rows / (\d+)\) nseg = rows / \d+;', 'fir_resample2_sep: rows per segment')
    assert len(re.findall(r'const dim3 grid\(shg_cdiv\(p\.nitem, 4\)\);', s)) == 3, 'marching kernels: four items per workgroup'
    s = _src('conv_wgrad.hip')
    c['WGRAD_WG'], a, b = _scan(s, r'long s = \(\(taps > 1 \? (\d+) : (\d+) \* (\d+)\) \+ tiles - 1\) / tiles;', 'wgrad_slices: workgroup target')
    c['WGRAD_WG_1X1'] = a * b
    c['WGRAD_MAX_SLICES'], b = _scan(s, r'if \(s > nchunk\) s = nchunk;\n\s*if \(s > (\d+)\) s = (\d+);', 'wgrad_slices: slice cap')
    assert c['WGRAD_MAX_SLICES'] == b
    m = re.search(r'const long cap = \((\d+)L << (\d+)\) / per_slice;', s)
    c['WGRAD_BYTES_CAP'] = (int(m.group(1)) << int(m.group(2))) if m else None            # None: the source has no byte cap on the partial sums
    s = _src('conv_wgrad_wino.hip')
    c['WGW_BO'], c['WGW_BI'] = _scan(s, r'namespace wgw \{[^}]*?constexpr int BO = (\d+), BI = (\d+);', 'wgw::BO, BI')
    c['WGW_WG'], = _scan(s, r'long s = \((\d+) \+ blocks - 1\) / blocks;', 'wgw_slices: workgroup target')
    c['WGW_MAX_SLICES'], b = _scan(s, r'if \(s > nchunk\) s = nchunk;\n\s*if \(s > (\d+)\) s = (\d+);', 'wgw_slices: slice cap')
    assert c['WGW_MAX_SLICES'] == b
    s = _src('optim.hip')
    c['OPT_THREADS'], = _scan(s, r'constexpr int OPT_THREADS = (\d+);', 'OPT_THREADS')
    c['OPT_VPT'], = _scan(s, r'constexpr int OPT_VPT = (\d+);', 'OPT_VPT')
    c['OPT_MAX_BLOCKS'], = _scan(s, r'constexpr int OPT_MAX_BLOCKS = (\d+);', 'OPT_MAX_BLOCKS')
    assert len(re.findall(r'const int grid = \(int\)\(chunks < OPT_MAX_BLOCKS \? chunks : OPT_MAX_BLOCKS\);', s)) == 2, 'optim: grid of both kernels'
    c['OPT_CHUNK'] = c['OPT_THREADS'] * c['OPT_VPT'] * 4
    # the rounding of the slice lengths: the plans below restate these lines, a floor in place of a cdiv (slices dropped or run past the
    # workspace) must not go unnoticed
    for name, n, line in (
            ('conv_mfma.hip', 1, 'p.i_per_slice = shg_cdiv(chunks, ks) * KC;'), ('conv_mfma.hip', 1, 'p.ksplit = shg_cdiv(p.I, p.i_per_slice);'),
            ('conv_mfma.hip', 1, 'p.tail_ks = tk; p.tail_ips = shg_cdiv(chunks, tk) * KC;'), ('conv_mfma.hip', 1, 'const int tail = nwork % slots;'),
            ('wino_common.h', 1, '*cps = shg_cdiv(nchunk, ks);'), ('wino_common.h', 1, 'ks = shg_cdiv(nchunk, *cps);'),
            ('conv_wgrad.hip', 3, 'const int per = (p.nchunk + p.nslice - 1) / p.nslice;'),
            ('conv_wgrad.hip', 3, 'const int c_begin = slice * per, c_end = min(p.nchunk, c_begin + per);'),
            ('conv_wgrad_wino.hip', 1, 'const int per = (p.nchunk + p.nslice - 1) / p.nslice;'),
            ('conv_wgrad_wino.hip', 1, 'const int c_begin = slice * per, c_end = min(p.nchunk, c_begin + per);'),
            ('upfirdn2d.hip', 1, 'const int cov_w = p.pl_pp > 0 ? 2 * p.pl_pp : p.OW, cov_h = p.pl_pp > 0 ? 2 * p.pl_ph2 : p.OH;'),
            ('conv_wino_poly.hip', 1, 'shg_wino_split('),          # the up launch splits; the down launch (no workspace argument) never does
            ('upfirdn2d.hip', 2, 'for (; nc < p.NC; nc += gridDim.z) {')):
        assert _src(name).count(line) == n, f'launch-plan scan: {name} no longer has {n} x "{line}"'
    return c


# ------------------------------------------------------------------------------------------------
# conv_mfma.hip
# ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def conv_instantiations():
    """The set of conv_mfma_kernel instantiations conv_dispatch can launch, as tuples of their template arguments (bools as 0 / 1)."""
    out = set()
    for m in re.finditer(r'launch_conv<([^>]+)>\(p, workspace', _src('conv_mfma.hip')):
        out.add(tuple({'true': 1, 'false': 0}.get(t.strip(), t.strip()) if not t.strip().isdigit() else int(t) for t in m.group(1).split(',')))
    return out


def inst(name):
    """'conv_mfma_kernel<9, 8, 2, 2, 2, 4, 1, false, true, 2>' (the spelling of the route tables) -> its tile constants; the instantiation
    must be one conv_dispatch launches."""
    args = name[name.index('<') + 1:name.rindex('>')].split(',')
    t = tuple({'true': 1, 'false': 0}[a.strip()] if a.strip() in ('true', 'false') else int(a) for a in args)
    assert t in conv_instantiations(), f'{name} is not launched by conv_dispatch'
    ntaps, kc, mo, np_, wo, wp, xq, up, db, occ = t
    return dict(NTAPS=ntaps, KC=kc, BO=mo * 32 * wo, BP=np_ * 32 * wp, NT=wo * wp * 64, XQ=xq, UP=bool(up), DB=bool(db), OCC=occ, args=t)


def tile_search(NB, rows, cols, BP, wgroups, S, span_y, span_x, patch_cap):
    """conv_mfma.hip tile_search: the tile class of one rows x cols region.  ``fallback``: nothing fitted the staging capacity."""
    c = constants()
    best, bpatch, btw, bth, btn, bfull = -1, 0, 1, 1, 1, 0
    for tw in range(1, min(cols, BP) + 1):
        if tw < c['TW_MIN'] and tw != cols and cols >= c['TW_MIN']:
            continue
        th = min(BP // tw, rows)
        pw = (tw - 1) * S + span_x
        while th > 1 and ((th - 1) * S + span_y) * pw > patch_cap:
            th -= 1
        tn = min(BP // (tw * th), NB)
        if wgroups > 1:
            tn = 1
        tn = max(tn, 1)
        while tn > 1 and tn * ((th - 1) * S + span_y) * pw > patch_cap:
            tn -= 1
        patch = tn * ((th - 1) * S + span_y) * pw
        if patch > patch_cap:
            continue
        tiles = cdiv(cols, tw) * cdiv(rows, th) * cdiv(NB, tn)
        full = 1 if tw % c['TW_FULL'] == 0 else 0
        if best < 0 or tiles < best or (tiles == best and (full > bfull or (full == bfull and patch < bpatch))):
            best, bpatch, btw, bth, btn, bfull = tiles, patch, tw, th, tn, full
    fallback = best < 0
    if fallback:
        btw, bth, btn = min(cols, c['TW_FALLBACK']), 1, 1
    t = dict(TW=btw, TH=bth, TN=btn, tiles_x=cdiv(cols, btw), tiles_y=cdiv(rows, bth), rows=rows, cols=cols, oy_base=0, ox_base=0, fallback=fallback,
             th_unshrunk=min(BP // btw, rows))
    t['n_tiles'] = t['tiles_x'] * t['tiles_y'] * cdiv(NB, btn)
    t['PH'], t['PW'] = (bth - 1) * S + span_y, (btw - 1) * S + span_x
    t['PATCH'] = btn * t['PH'] * t['PW']
    return t


def conv_geometry(H, W, k, mode, pad):
    """(OHp, OWp, S, span): the grid a launch computes (conv_fill).  mode 0 same / stride 1, 1 stride 2, 2 transposed stride 2."""
    if mode == 2:
        return H + 1, W + 1, 1, 2
    S = 1 if mode == 0 else 2
    return (H + 2 * pad - k) // S + 1, (W + 2 * pad - k) // S + 1, S, k


def conv_tiles(NB, H, W, OHp, OWp, S, span, O, BO, BP, up, patch_cap, wgroups=1):
    if not up:
        cls = [tile_search(NB, OHp, OWp, BP, wgroups, S, span, span, patch_cap)]
    else:
        cls = [tile_search(NB, H, W, BP, wgroups, 1, 2, 2, patch_cap), tile_search(NB, 1, W + 1, BP, wgroups, 1, 2, 2, patch_cap),
               tile_search(NB, H, 1, BP, wgroups, 1, 2, 2, patch_cap)]
        cls[1]['oy_base'], cls[2]['ox_base'] = H, W
    return cls, sum(t['n_tiles'] for t in cls), cdiv(O, BO)


def conv_ksplit(grid, chunks, allow=True):
    c = constants()
    ks = 1
    while allow and grid * ks < c['KS_FILL'] and chunks // (ks * 2) >= c['KS_MIN_CHUNKS'] and ks < c['KS_MAX']:
        ks *= 2
    return ks


def conv_dispatch(O, OHp, OWp, k, mode, wgroups=1, in_scale=False, raw_out=False):
    """The template arguments conv_dispatch picks (the tap-list kernels; the 1x1 GEMM form is not a launch_conv)."""
    c = constants()
    narrow = O <= 64
    if mode == 2:
        big = OWp >= c['CONV_UP_MIN'] and OHp >= 16 and wgroups == 1
        if big and raw_out:
            return (9, 8, 1, 1, 2, 8, 1, 1, 1, 4) if narrow else (9, 8, 1, 1, 4, 4, 1, 1, 1, 4)
        if big:
            return (9, 8, 2, 1, 1, 8, 1, 1, 1, 2) if narrow else (9, 8, 2, 1, 2, 4, 1, 1, 1, 2)
        return (9, 8, 2, 1, 1, 4, 2, 1, 0, 2)
    if k == 3 and mode == 0:
        if not narrow and OWp >= 32 and OHp >= 8 and wgroups == 1:
            return (9, 8, 2, 2, 2, 4, 1, 0, 1, 2)
        return (9, 8, 2, 2, 1, 4, 2, 0, 0, 3) if narrow else (9, 8, 2, 2, 2, 2, 2, 0, 0, 2)
    if k == 3 and mode == 1:
        if not narrow and OWp >= 32 and OHp >= 8 and wgroups == 1 and not in_scale:
            return (9, 8, 1, 2, 4, 4, 2, 0, 1, 4)
        return (9, 8, 2, 2, 1, 4, 5, 0, 0, 2) if narrow else (9, 8, 2, 2, 2, 2, 3, 0, 0, 2)
    assert k == 1 and mode == 0
    return (1, 32, 2, 2, 1, 4, 1, 0, 0, 3) if narrow else (1, 32, 2, 2, 2, 2, 1, 0, 0, 3)


def conv_plan(NB, I, O, H, W, k, mode, pad, t, cus, ws_bytes=None, wgroups=1, planar=True):
    """launch_conv for the instantiation ``t`` (from ``inst``) on a device of ``cus`` compute units.  ws_bytes: None = the workspace
    shg_conv2d_workspace_bytes asks for (what kernels.conv2d passes), 0 = no workspace, else the bytes given."""
    c = constants()
    OHp, OWp, S, span = conv_geometry(H, W, k, mode, pad)
    up = mode == 2
    assert up == t['UP']
    out_elems = 4 * NB * O * (H + 1) * (W + 1) if (up and planar) else NB * O * ((2 * H + 1) * (2 * W + 1) if up else OHp * OWp)
    if ws_bytes is None:
        ws_bytes = conv_workspace_bytes(NB, I, O, H, W, k, mode, pad, wgroups)
    have_ws = ws_bytes > 0
    cls, n_ptiles, n_otiles = conv_tiles(NB, H, W, OHp, OWp, S, span, O, t['BO'], t['BP'], up, t['XQ'] * t['NT'], wgroups)
    nwork = n_ptiles * n_otiles
    chunks = cdiv(I, t['KC'])
    ks_planned = conv_ksplit(nwork, chunks, have_ws)
    if t['DB'] and nwork >= cus:
        ks_planned = 1
    ks = ks_planned
    halvings = 0
    while ks > 1 and ks * out_elems * 4 > ws_bytes:
        ks //= 2
        halvings += 1
    i_per_slice = cdiv(chunks, ks) * t['KC']
    ksplit = cdiv(I, i_per_slice)
    tail_first, tail_ks, tail_ips, n_tail, tail = nwork, 1, I, 0, 0
    rule60 = None
    if t['DB'] and ksplit == 1 and have_ws:
        slots = cus
        tail = nwork % slots
        rule60 = tail * c['TAIL_NUM'] < slots * c['TAIL_DEN']
        if nwork > slots and tail > 0 and rule60:
            tk = 1
            while tk < c['TAIL_KS_MAX'] and tail * tk * 2 <= slots and chunks // (tk * 2) >= c['TAIL_MIN_CHUNKS']:
                tk *= 2
            need = tail * tk * (t['BO'] * t['BP'] * (4 if up else 1)) * 4
            if tk > 1 and need <= ws_bytes:
                n_tail, tail_first, tail_ks, tail_ips = tail, nwork - tail, tk, cdiv(chunks, tk) * t['KC']
    grid = nwork * ksplit if ksplit > 1 else tail_first + n_tail * tail_ks
    rg = min(cdiv(out_elems, 256), c['SPLITK_REDUCE_CAP']) if ksplit > 1 else 0
    return dict(cls=cls, n_ptiles=n_ptiles, n_otiles=n_otiles, nwork=nwork, chunks=chunks, ks_planned=ks_planned, ks=ks, halvings=halvings,
                i_per_slice=i_per_slice, ksplit=ksplit, tail=tail, rule60=rule60, tail_first=tail_first, tail_ks=tail_ks, tail_ips=tail_ips,
                n_tail=n_tail, grid=grid, launches=1 + (1 if n_tail else 0), reduce_grid=rg, out_elems=out_elems, BO=t['BO'], O=O, NB=NB,
                tn_max=max(q['TN'] for q in cls if q['n_tiles']), ws_bytes=ws_bytes)


def work_rect(plan, work):
    """Work item -> (o0, o1, n0, n1, oy0, oy1, ox0, ox1, class): the output channels, images and pixel rectangle (of the launch grid: for the
    transposed mode the (H+1) x (W+1) phase grid) it owns, clipped to the tensor."""
    otile, ptile = divmod(work, plan['n_ptiles'])
    ci = 0
    while ptile >= plan['cls'][ci]['n_tiles']:
        ptile -= plan['cls'][ci]['n_tiles']
        ci += 1
    t = plan['cls'][ci]
    txb, tyb, tnb = ptile % t['tiles_x'], (ptile // t['tiles_x']) % t['tiles_y'], ptile // (t['tiles_x'] * t['tiles_y'])
    oy0, ox0 = t['oy_base'] + tyb * t['TH'], t['ox_base'] + txb * t['TW']
    return (otile * plan['BO'], min((otile + 1) * plan['BO'], plan['O']), tnb * t['TN'], min((tnb + 1) * t['TN'], plan['NB']),
            oy0, min(oy0 + t['TH'], t['oy_base'] + t['rows']), ox0, min(ox0 + t['TW'], t['ox_base'] + t['cols']), ci)


def conv_workspace_bytes(NB, I, O, H, W, k, mode, pad, wgroups=1):
    """shg_conv2d_workspace_bytes."""
    c = constants()
    if NB < 1 or I < 1 or O < 1:
        return 0
    wgroups = max(wgroups, 1)
    if mode == 2:
        big = W + 1 >= c['CONV_UP_MIN'] and H + 1 >= 16 and wgroups == 1
        bo, bp = ((64, 256) if O <= 64 else (128, 128)) if big else (64, 128)
        _, n_ptiles, n_otiles = conv_tiles(NB, H, W, H + 1, W + 1, 1, 2, O, bo, bp, True, 512, wgroups)
        ks = conv_ksplit(n_ptiles * n_otiles, cdiv(I, 8))
        split = ks * 4 * NB * O * (H + 1) * (W + 1) * 4 if ks > 1 else 0
        return max(split, c['TAIL_WS_UP'] if big else 0)
    OH, OW, S, span = conv_geometry(H, W, k, mode, pad)
    if OH < 1 or OW < 1:
        return 0
    narrow = O <= 64
    KC = 8 if k == 3 else 32
    xq = 1 if k == 1 else (2 if S == 1 else (5 if narrow else 3))
    _, n_ptiles, n_otiles = conv_tiles(NB, H, W, OH, OW, S, span, O, 64 if narrow else 128, 256 if narrow else 128, False, xq * 256, wgroups)
    ks = conv_ksplit(n_ptiles * n_otiles, cdiv(I, KC))
    db = k == 3 and not narrow and OW >= 32 and OH >= 8
    if db:
        _, n_ptiles, n_otiles = conv_tiles(NB, H, W, OH, OW, S, span, O, 128, 256, False, xq * 256, wgroups)
        ks = max(ks, conv_ksplit(n_ptiles * n_otiles, cdiv(I, KC)))
    if ks > 1:
        return ks * NB * O * OH * OW * 4
    return c['TAIL_WS'] if db else 0


# ------------------------------------------------------------------------------------------------
# wino_common.h (conv_wino.hip, conv_wino4.hip)
# ------------------------------------------------------------------------------------------------

def wino_ksplit(tiles, nchunk):
    c = constants()
    ks = 1
    while tiles * ks < c['WINO_FILL'] and nchunk // (ks * 2) >= c['WINO_MIN_CHUNKS']:
        ks *= 2
    return ks


def wino_split(tiles, nchunk, out_bytes, ws_bytes, aligned16=True):
    """shg_wino_split -> dict(ks_planned, halvings, cps, ks, last): ``last`` = chunks of the last slice."""
    ks0 = wino_ksplit(tiles, nchunk) if (ws_bytes > 0 and aligned16) else 1
    ks, halvings = ks0, 0
    while ks > 1 and ks * out_bytes > ws_bytes:
        ks //= 2
        halvings += 1
    cps = cdiv(nchunk, ks)
    ks2 = cdiv(nchunk, cps)
    return dict(ks_planned=ks0, halvings=halvings, ks_fit=ks, cps=cps, ks=ks2, last=nchunk - (ks2 - 1) * cps)


def wino_tiles(kind, NB, I, OP, H, W):
    """(workgroups, nchunk, KC) of conv_wino ('wino') / conv_wino4 ('wino4', shipped route) for this problem."""
    c = constants()
    if kind == 'wino':
        wide = W >= c['WINO_WIDE_W']
        tx, ty = cdiv(W, c['WINO_TW_WIDE'] if wide else c['WINO_TW']), cdiv(H, c['WINO_TH_WIDE'] if wide else c['WINO_TH'])
        return tx * ty * NB * (OP // 64), cdiv(I, c['WINO_KC']), c['WINO_KC']
    assert kind == 'wino4'
    narrow = I >= c['URING_WIDE_MIN_I']
    shape = 2 if (W >= c['W4_S2_W'] and H >= c['W4_S2_H'] and not (narrow and H >= c['W4_S2_NARROW_H'])) else (
        1 if (W >= c['W4_S1_W'] and H >= c['W4_S1_H']) else 0)
    return cdiv(W, c['W4_TW'] << shape) * cdiv(H, c['W4_TH'] >> shape) * NB * (OP // 64), cdiv(I, c['WINO4_KC']), c['WINO4_KC']


def wino_workspace_bytes(kind, NB, I, O, OP, H, W):
    """shg_conv2d_wino_workspace_bytes / shg_conv2d_wino4_workspace_bytes."""
    if NB < 1 or I < 1 or O < 1 or OP < 64 or H < 1 or W < 1:
        return 0
    tiles, nchunk, _ = wino_tiles(kind, NB, I, OP, H, W)
    ks = wino_ksplit(tiles, nchunk)
    return ks * NB * O * H * W * 4 if ks > 1 else 0


def up_poly_tiles(NB, I, OP, H, W):
    """conv_wino_poly.hip up_poly_plan: (workgroups of the two Winograd schemes that shg_wino_split counts, nchunk, KC)."""
    c = constants()
    bwide = W >= 32
    nby, nbx = H // 2, W // 2
    b = cdiv(nbx, 16 if bwide else 8) * cdiv(nby, 4 if bwide else 8) * NB
    aby, abx = cdiv(H + 1, 3), cdiv(W + 1, 3)
    flat = bwide and abx in (11, 22, 43)
    wide = bwide and cdiv(abx, 16) * cdiv(aby, 4) < cdiv(abx, 8) * cdiv(aby, 8)
    a = (cdiv(aby * abx, 64) if flat else cdiv(abx, 16 if wide else 8) * cdiv(aby, 4 if wide else 8)) * NB
    return (a + b) * (OP // 64), cdiv(I, c['POLY_KC']), c['POLY_KC']


def up_poly_supported(NB, I, O, H, W):
    return H >= 16 and W >= 16 and H % 2 == 0 and W % 4 == 0 and I <= 128 * constants()['POLY_KC'] and NB >= 1 and O >= 1


def up_poly_workspace_bytes(NB, I, O, OP, H, W):
    """shg_conv2d_up_poly_workspace_bytes."""
    if not up_poly_supported(NB, I, O, H, W) or OP < 64:
        return 0
    tiles, nchunk, _ = up_poly_tiles(NB, I, OP, H, W)
    ks = wino_ksplit(tiles, nchunk)
    return ks * 4 * NB * O * (H + 1) * (W + 1) * 4 if ks > 1 else 0


def wino_reduce_grid(NB, O, H, W):
    total = NB * O * H * W
    return min((total // 4 + 255) // 256, constants()['WINO_REDUCE_CAP'])


# ------------------------------------------------------------------------------------------------
# upfirdn2d.hip
# ------------------------------------------------------------------------------------------------

def fir_out(H, W, fh, fw, up, down, pad):
    return (H * up + pad[2] + pad[3] - fh + down) // down, (W * up + pad[0] + pad[1] - fw + down) // down


def fir_same_plan(NC, OH, OW, ph2=0, pp=0):
    """ufd_launch, the 4x4 'same' kernel: planes per grid, trips per workgroup.  pp > 0: the planar-output form (shg_fir_down_planar_f32), whose
    grid covers the whole 2 pp x 2 ph2 extent of the phase planes, padding included."""
    c = constants()
    if pp > 0:
        OW, OH = 2 * pp, 2 * ph2
    tiles = cdiv(OW, c['FIR_SAME_TW']) * cdiv(OH, c['FIR_SAME_TH'])
    gzs = min(max(c['FIR_SAME_WG'] // tiles, 1), NC)
    return dict(tiles=tiles, gzs=gzs, trips=cdiv(NC, gzs), last_trip=NC - (cdiv(NC, gzs) - 1) * gzs)


def fir_generic_plan(NC, OH, OW):
    c = constants()
    gz = min(NC, c['FIR_GENERIC_GZ'])
    return dict(gz=gz, grid=(cdiv(OW, c['FIR_GENERIC_TW']), cdiv(OH, c['FIR_GENERIC_TH']), gz), trips=cdiv(NC, gz), last_trip=NC - (cdiv(NC, gz) - 1) * gz)


def fir_strided_plan(total):
    c = constants()
    blocks = min((total + 255) // 256, c['FIR_STRIDED_CAP'])
    return dict(blocks=blocks, trips=cdiv(total, blocks * 256))


def fir_up_planar_plan(NC, H, W):
    """shg_upfir_planar_f32 (H, W the low-resolution extents)."""
    c = constants()
    w0, t0, w1, t1, t2, area = c['FIR_UP_TV']
    TV = t0 if W >= w0 else (t1 if W >= w1 else t2)
    TU = area // TV
    tiles = cdiv(W, TV) * cdiv(H, TU)
    gz = min(max(c['FIR_UP_WG'] // tiles, 1), NC)
    return dict(TV=TV, TU=TU, tiles=tiles, gz=gz, trips=cdiv(NC, gz), last_trip=NC - (cdiv(NC, gz) - 1) * gz)


def march_plan(kind, NC, H, W, wide=False):
    """The row-marching kernels: kind 'down' (shg_fir_pad2_sep_f32; ``wide``: the march4 form), 'up' (shg_upfir_planar_sep_f32, H / W the
    low-resolution extents), 'dn2' / 'up2' (shg_fir_resample2_sep_f32) -> plane groups, row segments, items, grid."""
    c = constants()
    if kind == 'down':
        lpg = 64 if wide else min(W, 64)
        rows, per = H + 1, c['MARCH_ROWS_DOWN']
    elif kind == 'up':
        lpg = min(W // 2, 64)
        rows, per = H, c['MARCH_ROWS_UP']
    else:
        lanes = W // 4 if kind == 'dn2' else W // 2
        lpg = min(lanes, 64)
        rows, per = (H // 2 if kind == 'dn2' else H), c['MARCH_ROWS_RS']
    G = 1 if (kind == 'down' and wide) else 64 // lpg
    npg = cdiv(NC, G)
    nseg = max(min(cdiv(c['MARCH_WAVES'], npg), rows // per), 1)
    R = cdiv(rows, nseg)
    nseg = cdiv(rows, R)
    nitem = npg * nseg
    return dict(G=G, npg=npg, R=R, nseg=nseg, nitem=nitem, grid=cdiv(nitem, 4), rows=rows)


# ------------------------------------------------------------------------------------------------
# conv_wgrad.hip, conv_wgrad_wino.hip
# ------------------------------------------------------------------------------------------------

def wgrad_slices(NB, I, O, OH, OW, taps, with_cap=True):
    """wgrad_slices.  ``with_cap=False``: without the byte cap on the partial sums (a source without that cap has WGRAD_BYTES_CAP None)."""
    c = constants()
    tiles = cdiv(I, 64) * cdiv(O, 64)
    nchunk = NB * OH * cdiv(OW, 32)
    s = cdiv(c['WGRAD_WG'] if taps > 1 else c['WGRAD_WG_1X1'], tiles)
    if with_cap and c['WGRAD_BYTES_CAP'] is not None:
        s = min(s, c['WGRAD_BYTES_CAP'] // (O * I * taps * 4))
    s = min(s, nchunk, c['WGRAD_MAX_SLICES'])
    return max(s, 1)


def wgrad_workspace_bytes(NB, I, O, OH, OW, k):
    """shg_conv2d_wgrad_workspace_bytes."""
    s = wgrad_slices(NB, I, O, OH, OW, k * k)
    need = s * O * I * k * k * 4 if s > 1 else 0
    thin = 0
    hw = OH * OW
    if k == 1 and not (I > 8 and O > 8) and hw % 1024 == 0:
        chunks = NB * (hw // 4096 if hw % 4096 == 0 else hw // 1024)
        thin = (chunks if chunks <= 8192 else 0) * O * I * 4
    return max(thin, need)


def wgrad_chunks(NB, I, O, H, W, OH, OW, k, stride, pad):
    """-> dict(kernel, px, rows, nchunk, nslice, per, last, H, W, OH, OW): the geometry the launch settles on (1x1 layers of whole 64-channel
    tiles are flattened to one row of H W pixels), ``per`` chunks per slice, ``last`` chunks of the last slice that has any."""
    chan64 = pad == 0 and I % 64 == 0 and O % 64 == 0 and 64 * H * W < (1 << 31) and 2 * OH * OW < (1 << 31)
    full_rows = 0
    if chan64 and k == 3 and stride == 2 and OW in (16, 8) and W == 2 * OW + 1 and (OH - 1) * 2 + 2 < H and OH % (32 // OW) == 0:
        full_rows = 32 // OW
    if chan64 and k == 1 and stride == 1 and H == OH and W == OW and (H * W) % 64 == 0:
        H, W = 1, H * W
        OH, OW = 1, W
    px_packed = 64 if stride == 1 else 32
    packed = (not full_rows and k == 3 and 4 <= OW <= px_packed // 4 and OW & (OW - 1) == 0 and OH & (OH - 1) == 0 and W <= OW * stride + 2
              and pad <= 2)
    two_rows = not packed and k == 3 and stride == 1 and OW == 32 and OH % 2 == 0 and W == 32 + 2 - 2 * pad
    px = 64 if stride == 1 else 32
    full = (not packed and not two_rows and not full_rows and chan64 and OW % px == 0 and (OH - 1) * stride + k - 1 < H
            and (OW - px) * stride + 63 + (k - stride if k > stride else 0) < W)
    chunks_x = 1 if full_rows else cdiv(OW, px)
    if full_rows:
        nchunk = NB * (OH // full_rows)
    elif packed:
        nchunk = cdiv(NB * OH * OW, px)
    elif two_rows:
        nchunk = NB * (OH // 2)
    else:
        nchunk = NB * OH * chunks_x
    nslice = min(wgrad_slices(NB, I, O, OH, OW, k * k), nchunk)
    per = cdiv(nchunk, nslice)
    used = cdiv(nchunk, per)
    if packed:
        kern = f'conv_wgrad_packed_kernel<3, 3, {stride}>'
    elif two_rows:
        kern = 'conv_wgrad_kernel<3, 3, 1, 2>'
    elif full_rows:
        kern = f'conv_wgrad_full_kernel<3, 3, 2, {full_rows}>'
    elif full:
        kern = f'conv_wgrad_full_kernel<{k}, {k}, {stride}, 1>'
    else:
        kern = f'conv_wgrad_kernel<{k}, {k}, {stride}, 1>'
    return dict(kernel=kern, px=px, chunks_x=chunks_x, nchunk=nchunk, nslice=nslice, per=per, used=used, last=nchunk - (used - 1) * per,
                H=H, W=W, OH=OH, OW=OW, packed=packed, two_rows=two_rows, full_rows=full_rows)


def wgw_plan(NB, I, O, H, W):
    """conv_wgrad_wino.hip wgw_slices and the chunk grid of shg_conv2d_wgrad_wino_f32."""
    c = constants()
    lx = 3 if W >= 32 else (2 if W >= 16 else (1 if W >= 8 else 0))
    ty = (8 if lx >= 2 else 4) >> lx
    blocks = cdiv(I, c['WGW_BI']) * cdiv(O, c['WGW_BO'])
    cty, ctx = cdiv(H, 4 * ty), cdiv(W, 4 << lx)
    nchunk = NB * cty * ctx
    s = max(min(cdiv(c['WGW_WG'], blocks), nchunk, c['WGW_MAX_SLICES']), 1)
    per = cdiv(nchunk, s)
    used = cdiv(nchunk, per)
    return dict(lx=lx, rows=4 * ty, cols=4 << lx, cty=cty, ctx=ctx, nchunk=nchunk, nslice=s, per=per, used=used, last=nchunk - (used - 1) * per,
                ws_bytes=s * O * I * 9 * 4 if s > 1 else 0)


# ------------------------------------------------------------------------------------------------
# optim.hip
# ------------------------------------------------------------------------------------------------

def opt_grid(chunks):
    c = constants()
    grid = min(chunks, c['OPT_MAX_BLOCKS'])
    return dict(grid=grid, trips=cdiv(chunks, grid))
