"""tests/alloc_fill.py on CPU tensors (no GPU): the three patterns per dtype family, what passes through, what is restored, what is recorded."""
import numpy as np
import pytest
import torch

import alloc_fill
from alloc_fill import filled

FLOATS = (torch.float16, torch.bfloat16, torch.float32, torch.float64)
BIG = {torch.float16: 61280.0, torch.float32: 1.3e36, torch.float64: 6.5e286}     # 0x7B7B, 0x7B7B7B7B, 0x7B7B7B7B7B7B7B7B


def _bytes(t):
    return np.frombuffer(bytes(t.untyped_storage()), np.uint8)


@pytest.mark.parametrize('dtype', FLOATS)
def test_floating_patterns(dtype):
    with filled('zero'):
        z = torch.empty(3, 5, dtype=dtype)
    with filled('nan'):
        n = torch.empty(3, 5, dtype=dtype)
    with filled('big'):
        b = torch.empty(3, 5, dtype=dtype)
    assert bool((z == 0).all()) and not _bytes(z).any()
    assert bool(torch.isnan(n).all()) and bool((_bytes(n) == 0xFF).all())
    assert bool((_bytes(b) == 0x7B).all()) and bool(torch.isfinite(b).all()) and bool((b == b.view(-1)[0]).all())
    if dtype in BIG:
        assert abs(float(b.view(-1)[0]) / BIG[dtype] - 1) < 0.02, float(b.view(-1)[0])
    else:
        assert float(b.view(-1)[0]) > 1e36


@pytest.mark.parametrize('dtype', (torch.uint8, torch.int8))
def test_byte_integer_patterns(dtype):
    for pattern, byte in (('zero', 0x00), ('nan', 0xFF), ('big', 0x7B)):
        with filled(pattern):
            t = torch.empty(7, dtype=dtype)
        assert bool((_bytes(t) == byte).all()), pattern


@pytest.mark.parametrize('dtype', (torch.int16, torch.int32, torch.int64))
def test_wide_integer_patterns_are_small_values(dtype):
    for pattern, value in (('zero', 0), ('nan', 1), ('big', 2)):
        with filled(pattern):
            t = torch.empty(2, 3, dtype=dtype)
        assert t.tolist() == [[value] * 3] * 2, pattern


def test_bool_stays_a_valid_bool():
    for pattern, value in (('zero', 0), ('nan', 1), ('big', 1)):
        with filled(pattern):
            t = torch.empty(5, dtype=torch.bool)
        assert bool((_bytes(t) == value).all()), pattern


def test_all_three_functions_fill_and_return_the_tensor_they_got():
    src = torch.zeros(2, 3, 4, 5).contiguous(memory_format=torch.channels_last)
    with filled('nan') as rec:
        a = torch.empty((4,))
        b = torch.empty_like(src)
        c = src.new_empty((2, 2))
        d = torch.empty_like(src, dtype=torch.float16)
    assert rec.count == 4
    for t in (a, b, c, d):
        assert bool(torch.isnan(t).all())
    assert b.is_contiguous(memory_format=torch.channels_last) and b.stride() == src.stride()
    assert d.dtype == torch.float16 and d.is_contiguous(memory_format=torch.channels_last)
    assert c.dtype == src.dtype and tuple(c.shape) == (2, 2)


def test_memory_format_and_pin_memory_pass_through():
    with filled('nan'):
        y = torch.empty((2, 8, 3, 5), dtype=torch.float16, memory_format=torch.channels_last)
        p = torch.empty(6, dtype=torch.int32, pin_memory=False)
    assert y.is_contiguous(memory_format=torch.channels_last) and y.stride() == (120, 1, 40, 8)
    assert bool(torch.isnan(y).all())
    assert p.tolist() == [1] * 6 and not p.is_pinned()
    with filled('big'):
        y = torch.empty((2, 8, 3, 5), dtype=torch.float32, memory_format=torch.channels_last)
    assert y.stride() == (120, 1, 40, 8) and bool((_bytes(y) == 0x7B).all())


def test_whole_storage_is_filled_not_only_the_view():
    """The fill covers the storage, not the elements the tensor's strides reach."""
    with filled('big'):
        t = torch.empty(10, dtype=torch.float32)
    assert t.untyped_storage().nbytes() == 40 and bool((_bytes(t) == 0x7B).all())


def test_zero_size_tensors_are_accepted():
    for pattern in alloc_fill.PATTERNS:
        with filled(pattern) as rec:
            a = torch.empty((0, 1, 32, 32))
            b = torch.empty(0, dtype=torch.int32)
            c = torch.empty_like(a)
            d = a.new_empty((0,))
        assert rec.count == 4 and a.numel() == b.numel() == c.numel() == d.numel() == 0


def test_functions_are_restored_after_an_exception():
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty, 'new_empty' in vars(torch.Tensor))
    with pytest.raises(ZeroDivisionError):
        with filled('nan'):
            assert torch.empty is not before[0] and torch.empty_like is not before[1] and torch.Tensor.new_empty is not before[2]
            1 / 0
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty, 'new_empty' in vars(torch.Tensor)) == before
    with filled('zero'):                                       # and the helper is usable again
        pass
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before[:3]


def test_nesting_raises_and_leaves_the_outer_fill_active():
    with filled('nan'):
        with pytest.raises(RuntimeError, match='re-entrant'):
            with filled('big'):
                pass
        assert bool(torch.isnan(torch.empty(3)).all())
    assert not bool(torch.isnan(torch.zeros(3)).any()) and torch.empty.__module__ != alloc_fill.__name__


def test_unknown_pattern_raises():
    with pytest.raises(ValueError):
        with filled('ones'):
            pass


def test_recorded_site_is_the_innermost_package_frame():
    import shgan_amd  # noqa: F401
    from shgan_amd import kernels, resize
    img = np.full((2, 3, 3), 7, np.uint8)
    with filled('nan') as rec:
        packed, shapes = resize.pack_images([img, img])
        torch.empty(3)                                         # from the test itself: no frame inside the package, not a site
    assert rec.sites == {('resize.py', 'pack_images')} and rec.count == 2
    assert bool((packed == 7).all()) and shapes.tolist() == [[2, 3, 0], [2, 3, 18]]
    # the pass-through allocators are looked through: an allocation belongs to the caller of _Launch.new
    with filled('big') as rec:
        t = kernels._Launch().new((2, 2))
    assert rec.count == 1 and rec.sites == set() and bool((_bytes(t) == 0x7B).all())
    assert ('kernels.py', 'new') in alloc_fill.WRAPPERS and ('kernels_f16.py', '_new_cl') in alloc_fill.WRAPPERS
