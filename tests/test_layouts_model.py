"""tests/layouts.py pinned on the host: scatter then gather is the identity, expect() differs from an all-poison buffer exactly on
the plane's pixels, no two pixels of a layout share an element, the named layouts are what their table says, and their extents
follow check_plane's rules (wm_api.hip): none of them is refused, one with a frame stride one short of a frame's extent is."""
import numpy as np
import pytest

import layouts as LY

SHAPES = [(70, 300), (40, 266), (64, 516), (5, 7)]
KINDS = [(1, 1, False), (3, 1, False), (1, 5, True), (3, 5, True), (1, 1, True), (3, 3, True)]  # (channels, frames, batched)


def array_of(rows, cols, channels, frames, batched, dtype, seed=0):
    shape = ((frames,) if batched else ()) + ((channels,) if channels > 1 else ()) + (rows, cols)
    rng = np.random.default_rng(seed)
    # (1 .. 80: no pixel equals a poison, 0x5A = 90 among them)
    return rng.integers(1, 81, size=shape).astype(dtype)


@pytest.mark.parametrize("name", LY.NAMES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_scatter_gather_and_poison(name, shape, kind, dtype):
    rows, cols = shape
    channels, frames, batched = kind
    npdt = np.float32 if dtype == "f32" else np.uint8
    arr = array_of(rows, cols, channels, frames, batched, npdt)
    length = LY.room(LY.NAMES, rows, cols, channels, frames)
    lay = LY.make(name, rows, cols, channels, frames, length)
    for poison in LY.POISON[dtype]:
        buf = LY.expect(arr, lay, poison, channels)
        assert buf.dtype == npdt and buf.shape == (length,)
        np.testing.assert_array_equal(LY.gather(buf, lay, arr.shape, channels), arr)
        blank = np.full(length, poison, npdt)
        differs = LY.raw(buf) != LY.raw(blank)
        idx = LY.indices(lay, frames, channels, rows, cols).reshape(-1)
        assert len(np.unique(idx)) == arr.size                      # no two pixels share an element
        assert idx.min() == lay.offset and idx.max() == LY.extent(lay, rows, cols, channels, frames) - 1 < length
        on = np.zeros(length, bool)
        on[idx] = True
        np.testing.assert_array_equal(differs, on)                  # exactly the plane's pixels, nothing else
    # the strides a torch view of the buffer gets are the layout's
    s = LY.view_strides(lay, arr.ndim, channels)
    assert len(s) == arr.ndim and s[-1] == 1 and s[-2] == lay.pitch
    if channels > 1:
        assert s[-3] == lay.channel_stride
    if batched:
        assert s[0] == lay.frame_stride


def test_raw_compares_nan_poison_as_equal():
    a = np.full(8, np.nan, np.float32)
    assert not (a == a).any() and (LY.raw(a) == LY.raw(a.copy())).all()
    b = a.copy()
    b[3] = 1.0
    assert (LY.raw(a) != LY.raw(b)).sum() == 1


def test_named_layouts_are_what_the_table_says():
    rows, cols = 40, 266
    r4 = 268
    assert LY.strides_of("dense", rows, cols, 3) == (0, cols, rows * cols, 3 * rows * cols)
    assert LY.strides_of("pitched", rows, cols, 3) == (8, r4 + 12, rows * (r4 + 12), 3 * rows * (r4 + 12))
    off, pitch, cs, fs = LY.strides_of("gapped", rows, cols, 3)
    assert (off, pitch, cs, fs) == (4, r4 + 4, rows * (r4 + 4) + 8, 3 * (rows * (r4 + 4) + 8) + 28)
    assert LY.strides_of("every_other", rows, cols, 3) == (off, pitch, cs, 2 * fs)
    assert LY.strides_of("odd", rows, cols, 1) == (1, cols + 5, rows * (cols + 5) + 1, rows * (cols + 5) + 1 + 3)
    assert LY.strides_of("odd_frames_only", rows, cols, 3) == (0, r4, rows * r4, 3 * rows * r4 + 3)
    # the path each is meant to take (wm.h: u8 planes need base, pitch and strides to be multiples of 4 bytes)
    for ch, F in ((1, 1), (1, 5), (3, 5)):
        for name in ("pitched", "gapped", "every_other"):
            lay = LY.make(name, rows, cols, ch, F)
            assert LY.vector_path(lay, 1, ch, F) and LY.vector_path(lay, 4, ch, F)
        lay = LY.make("odd", rows, cols, ch, F)
        assert not LY.vector_path(lay, 1, ch, F) and LY.vector_path(lay, 4, ch, F)
        lay = LY.make("odd_frames_only", rows, cols, ch, F)
        assert LY.vector_path(lay, 1, ch, F) == (F == 1)        # generic by the frame stride alone
    assert LY.vector_path(LY.make("dense", 70, 300, 1, 5), 1, 1, 5) and not LY.vector_path(LY.make("dense", 40, 266, 1, 5), 1, 1, 5)


@pytest.mark.parametrize("name", LY.NAMES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_extents_follow_check_plane(name, shape, kind):
    rows, cols = shape
    channels, frames, _ = kind
    lay = LY.make(name, rows, cols, channels, frames)
    assert not LY.refused(lay, rows, cols, channels, frames)
    assert lay.length == LY.extent(lay, rows, cols, channels, frames) <= LY.room([name], rows, cols, channels, frames)
    if frames > 1:
        frame_extent = (channels - 1) * (lay.channel_stride if channels > 1 else 0) + rows * lay.pitch
        assert not LY.refused(lay._replace(frame_stride=frame_extent), rows, cols, channels, frames)
        assert LY.refused(lay._replace(frame_stride=frame_extent - 1), rows, cols, channels, frames)
    if channels > 1:
        assert LY.refused(lay._replace(channel_stride=rows * lay.pitch - 1), rows, cols, channels, frames)
    assert LY.refused(lay._replace(pitch=cols - 1), rows, cols, channels, frames)


def test_room_holds_any_mix_of_strides():
    """a stride of one layout used with the others of another (a kernel with one word exchanged) stays inside room()"""
    rows, cols, channels, frames = 40, 266, 3, 6
    n = LY.room(LY.NAMES, rows, cols, channels, frames)
    s = [LY.strides_of(nm, rows, cols, channels) for nm in LY.NAMES]
    for a in s:
        for b in s:
            for swap in range(1, 4):
                mixed = list(a)
                mixed[swap] = b[swap]
                lay = LY.Layout(*mixed, n)
                assert LY.extent(lay, rows, cols, channels, frames) <= n - rows * max(v[1] for v in s)


def test_every_cell_of_the_coverage_table_is_filled():
    """the case lists of tests/test_gpu_layouts.py, call x plane role x layout: no cell of a role the call has is empty, and every
    call with more than one plane has a case in which all its planes differ (the table itself is printed for the record)"""
    import test_gpu_layouts as G
    cells, alldiff = G.coverage()
    calls = sorted({(c, r) for c, r, n in cells})
    for call, role in calls:
        row = [cells.get((call, role, n), 0) for n in LY.NAMES]
        print(f"{call:34s} {role:9s} " + " ".join(f"{n}={v}" for n, v in zip(LY.NAMES, row)))
        if call.startswith("fused"):
            continue   # (vector-path layouts only: the others cannot take the fused kernels)
        assert all(v > 0 for v in row), (call, role, row)
    for call in {c for c, r in calls if r in ("base", "mask_out")}:
        assert alldiff.get(call, 0) >= 1, call
