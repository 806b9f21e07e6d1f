"""CPU (no GPU): the host side of the Places2 device resize -- Pillow's bicubic coefficient tables and the two-pass integer reference
(resize.py) against ``Image.resize([R, R], BICUBIC)`` (FixResolutionLoader, ds_places2.py:90-103), the table / tiling invariants the
kernel relies on, and the argument checks of the C entry point."""
import ctypes

import numpy as np
import pytest

import shgan_amd  # noqa: F401
from shgan_amd import _lib
from shgan_amd import resize as rz


def _pillow(img, R):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.fromarray(img).resize([R, R], Image.BICUBIC)).transpose(2, 0, 1))


def _cases(rs, n):
    """(h, w, R), R in {256, 512}: down-scale factors 1..6 and up-sampling, equal sizes, one axis only, odd sizes."""
    out = []
    for i in range(n):
        R = int(rs.choice([256, 512]))
        lo, hi = [(0.2, 1.0), (1.0, 2.0), (2.0, 3.5), (3.5, 6.0)][i % 4]
        h, w = (max(1, int(R * rs.uniform(lo, hi))) | 1 if i % 2 else max(2, int(R * rs.uniform(lo, hi))) for _ in range(2))
        if i % 9 == 4:
            h = R
        if i % 10 == 7:
            w = R
        if i % 25 == 12:
            h = w = R
        out.append((h, w, R))
    return out


def test_reference_is_bit_identical_to_pillow():
    """>= 200 seeded cases; images of at most ~0.6 MPixel (the scale factors, not the absolute sizes, exercise the tables)."""
    rs = np.random.RandomState(7)
    cases = _cases(rs, 204)
    assert {c[2] for c in cases} == {256, 512} and any(h == w == R for h, w, R in cases)
    assert any(h == R and w != R for h, w, R in cases) and any(w == R and h != R for h, w, R in cases)
    for h, w, R in cases:
        if h * w > 600_000:                     # the big down-scales: a thinner image of the same factor along the long axis
            if h > w:
                w = max(1, 600_000 // h)
            else:
                h = max(1, 600_000 // w)
        img = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        want = _pillow(img, R)
        got = rz.resize_reference(img, R)
        assert np.array_equal(got, want), ((h, w, R), int((got != want).sum()))
        assert np.array_equal(rz.resize_reference(img, R, flip=True), want[:, :, ::-1])


@pytest.mark.parametrize('n_in,n_out,width', [(683, 512, 7), (300, 512, 5), (1311, 256, 23), (512, 512, 1), (1024, 512, 9)])
def test_table_width_bounds_and_headroom(n_in, n_out, width):
    bounds, k = rz.bicubic_coeffs(n_in, n_out)
    assert k.shape == (n_out, width) and bounds.shape == (n_out, 2) and k.dtype == np.int32
    xmin, n = bounds[:, 0], bounds[:, 1]
    assert (xmin >= 0).all() and (n >= 1).all() and (n <= width).all() and (xmin + n <= n_in).all()
    assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + n) >= 0).all()       # monotone: a band's source rows are one range
    taps = np.arange(width)[None, :] < n[:, None]
    assert (k[~taps] == 0).all()


def test_int32_headroom_over_scales():
    """sum |k| * 255 * ... < 2^31 for every output of every case: the kernel's int32 accumulator cannot overflow."""
    for n_in in list(range(1, 64)) + list(range(64, 4000, 37)):
        for R in (256, 512):
            _, k = rz.bicubic_coeffs(n_in, R)
            worst = (1 << 21) + 255 * np.abs(k.astype(np.int64)).sum(1).max()
            assert worst < 2 ** 31, (n_in, R)


def test_table_and_tiling_fit_the_kernel():
    shapes = np.array([(512, 683, 0), (3000, 400, 1), (90, 64, 2), (512, 512, 3)])
    for R in (256, 512, 37):
        table, chunks, bands, lds = rz.build_table(shapes, R, flip=[0, 1, 0, 1])
        assert table.dtype == np.int32 and 12 <= lds <= rz.LDS_BYTES
        desc = table[:len(shapes) * rz.DESC_INTS].reshape(-1, rz.DESC_INTS)
        assert list(desc[:, 3]) == [0, 1, 0, 1]
        for h, w, off, fl, hb, hk, kh, vb, vk, kv, tb, cw in desc:
            assert np.array_equal(table[hb:hb + 2 * R].reshape(R, 2), rz.bicubic_coeffs(w, R)[0])
            assert np.array_equal(table[hk:hk + R * kh].reshape(R, kh), rz.bicubic_coeffs(w, R)[1])
            assert np.array_equal(table[vk:vk + R * kv].reshape(R, kv), rz.bicubic_coeffs(h, R)[1])
            assert -(-R // tb) <= bands and -(-R // cw) <= chunks and (cw == R or cw % 4 == 0)
            vbnd = table[vb:vb + 2 * R].reshape(R, 2)
            for y0 in range(0, R, tb):
                y1 = min(y0 + tb, R)
                span = vbnd[y1 - 1, 0] + vbnd[y1 - 1, 1] - vbnd[y0, 0]
                assert 3 * span * ((min(cw, R) + 3) // 4 * 4) <= lds


def test_pack_images_layout():
    rs = np.random.RandomState(2)
    imgs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in [(5, 7), (3, 3), (1, 9)]]
    packed, shapes = rz.pack_images(imgs)
    assert shapes.tolist() == [[5, 7, 0], [3, 3, 105], [1, 9, 132]] and packed.numel() == 159
    for im, (h, w, o) in zip(imgs, shapes.tolist()):
        assert np.array_equal(packed.numpy()[o:o + h * w * 3].reshape(h, w, 3), im)
    with pytest.raises(ValueError):
        rz.pack_images([np.zeros((4, 4), np.uint8)])


def test_c_entry_point_validates_its_arguments_without_a_gpu():
    lib = _lib.get_lib()
    f = lib.shg_resize_bicubic_u8
    P = ctypes.c_void_p(256)
    assert f(None, 100, P, 100, P, 1, 64, 1, 4, 1024, None) == -1 and b'null' in lib.shg_last_error()
    assert f(P, 100, P, 100, P, 0, 64, 1, 4, 1024, None) == -1 and b'B must' in lib.shg_last_error()
    assert f(P, 100, P, 100, P, 1, 0, 1, 4, 1024, None) == -1 and b'R must' in lib.shg_last_error()
    assert f(P, 2, P, 100, P, 1, 64, 1, 4, 1024, None) == -1 and b'src_bytes' in lib.shg_last_error()
    assert f(P, 1 << 31, P, 100, P, 1, 64, 1, 4, 1024, None) == -1 and b'src_bytes' in lib.shg_last_error()
    assert f(P, 100, P, 23, P, 2, 64, 1, 4, 1024, None) == -1 and b'descriptors' in lib.shg_last_error()
    assert f(P, 100, P, 100, P, 1, 64, 0, 4, 1024, None) == -1 and b'chunks' in lib.shg_last_error()
    assert f(P, 100, P, 100, P, 1, 64, 1, 65, 1024, None) == -1 and b'bands' in lib.shg_last_error()
    assert f(P, 100, P, 100, P, 1, 64, 1, 4, 49153, None) == -1 and b'lds_bytes' in lib.shg_last_error()
    with pytest.raises(_lib.ShgError):
        import torch
        rz.resize_bicubic_u8(torch.zeros(12, dtype=torch.uint8), [[2, 2, 0]], 4)
