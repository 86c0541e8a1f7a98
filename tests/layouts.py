"""A plane layout as data: where the pixels of a [R, C], [3, R, C], [F, R, C] or [F, 3, R, C] array lie in one flat buffer.

Plain numpy and torch; nothing here reads the library's own descriptors.  A Layout holds the element offset of the first pixel,
the pitch, the channel stride, the frame stride and the buffer's length, all in elements.  place() builds the buffer on the
device -- poison everywhere, the pixels scattered in -- and returns it with an as_strided view whose strides are the layout's, so
plane_of(view) is exactly that wm_plane; expect() builds the same buffer on the host.  A writing call is then checked on raw
bytes: the output buffer after the call must equal expect(result, layout, poison), which says "the right pixels in the right
place" and "not one byte written outside the plane" at once (raw(): f32 as int32, so a NaN poison equals itself)."""
from collections import namedtuple

import numpy as np

Layout = namedtuple("Layout", "offset pitch channel_stride frame_stride length")

NAMES = ("dense", "pitched", "gapped", "every_other", "odd", "odd_frames_only")

# two poisons per element type (wm.h: f32 pixels lie in [0, 255]): results must not depend on which one fills the padding
POISON = {"f32": (np.float32(np.nan), np.float32(-1e30)), "u8": (np.uint8(0xA5), np.uint8(0x5A))}


def roundup4(n):
    return (n + 3) // 4 * 4


def strides_of(name, rows, cols, channels=1):
    """(offset, pitch, channel_stride, frame_stride) of a named layout"""
    r4 = roundup4(cols)
    if name == "dense":          # the baseline: everything tight
        off, pitch = 0, cols
        cs = rows * pitch
        fs = channels * cs
    elif name == "pitched":      # FFmpeg's linesize: a multiple of 4, strides tight
        off, pitch = 8, r4 + 12
        cs = rows * pitch
        fs = channels * cs
    elif name in ("gapped", "every_other"):  # a frame pool with guard elements between channels and frames; buf[::2] of one
        off, pitch = 4, r4 + 4
        cs = rows * pitch + 8
        fs = channels * cs + 28
        if name == "every_other":
            fs *= 2
    elif name == "odd":          # nothing a multiple of 4: u8 planes leave the vector path, f32 rows are off 16 bytes
        off, pitch = 1, cols + 5
        cs = rows * pitch + 1
        fs = channels * cs + 3
    elif name == "odd_frames_only":  # base and pitch aligned, only the frame stride is off 4 bytes
        off, pitch = 0, r4
        cs = rows * pitch
        fs = rows * pitch * channels + 3
    else:
        raise KeyError(name)
    return off, pitch, cs, fs


def extent(lay, rows, cols, channels=1, frames=1):
    """elements from the buffer's start to the end of the last pixel"""
    return lay.offset + (frames - 1) * lay.frame_stride + (channels - 1) * lay.channel_stride + (rows - 1) * lay.pitch + cols


def room(names, rows, cols, channels=1, frames=1):
    """a buffer length that holds every named layout of a test and then some: the largest offset, pitch, channel stride and frame
    stride each taken on its own, plus one full plane of slack -- so an address formed from ANY mix of the test's strides (what a
    kernel with one stride exchanged for another plane's would form) still lies inside the buffer"""
    s = [strides_of(n, rows, cols, channels) for n in names]
    off, pitch, cs, fs = (max(v[i] for v in s) for i in range(4))
    return off + (frames - 1) * fs + (channels - 1) * cs + (rows - 1) * pitch + cols + rows * pitch


def make(name, rows, cols, channels=1, frames=1, length=None):
    off, pitch, cs, fs = strides_of(name, rows, cols, channels)
    lay = Layout(off, pitch, cs, fs, 0)
    need = extent(lay, rows, cols, channels, frames)
    if length is None:
        length = need
    assert length >= need, (name, length, need)
    return lay._replace(length=length)


def dims(arr, channels=1):
    """(frames, channels, rows, cols, batched) of an array of one of the four shapes"""
    nd = arr.ndim
    base = 2 if channels == 1 else 3
    assert nd in (base, base + 1) and (channels == 1 or arr.shape[-3] == channels), (arr.shape, channels)
    batched = nd == base + 1
    return (arr.shape[0] if batched else 1), channels, arr.shape[-2], arr.shape[-1], batched


def indices(lay, frames, channels, rows, cols):
    """int64 [F, ch, R, C]: the buffer index of every pixel"""
    f = np.arange(frames, dtype=np.int64)[:, None, None, None] * lay.frame_stride
    c = np.arange(channels, dtype=np.int64)[None, :, None, None] * lay.channel_stride
    r = np.arange(rows, dtype=np.int64)[None, None, :, None] * lay.pitch
    x = np.arange(cols, dtype=np.int64)[None, None, None, :]
    return lay.offset + f + c + r + x


def expect(arr, lay, poison, channels=1):
    """the host image of the buffer: `arr` in place, poison everywhere else"""
    arr = np.asarray(arr)
    F, ch, R, Cc, _ = dims(arr, channels)
    assert extent(lay, R, Cc, ch, F) <= lay.length
    buf = np.full(lay.length, poison, dtype=arr.dtype)
    buf[indices(lay, F, ch, R, Cc).reshape(-1)] = arr.reshape(-1)
    return buf


def gather(buf, lay, shape, channels=1):
    """the pixels of a host buffer laid out as `lay`, as an array of `shape`"""
    F, ch, R, Cc, _ = dims(np.empty(shape, np.uint8), channels)
    return np.asarray(buf)[indices(lay, F, ch, R, Cc).reshape(-1)].reshape(shape)


def view_strides(lay, ndim, channels=1):
    s = (lay.pitch, 1)
    if channels > 1:
        s = (lay.channel_stride,) + s
    if ndim == len(s) + 1:
        s = (lay.frame_stride,) + s
    return s


def view_of(buf, lay, shape, channels=1):
    """an as_strided view of a flat torch buffer whose strides are the layout's"""
    return buf.as_strided(tuple(shape), view_strides(lay, len(shape), channels), lay.offset)


def place(torch, arr, lay, poison, channels=1):
    """(flat device buffer, as_strided view of it): poison everywhere, `arr` scattered in"""
    buf = torch.from_numpy(expect(arr, lay, poison, channels)).cuda()
    return buf, view_of(buf, lay, np.shape(arr), channels)


def raw(a):
    """the bytes of a numpy array or torch tensor as a flat integer numpy array (f32 -> int32: NaN equals itself)"""
    if not isinstance(a, np.ndarray):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(a).reshape(-1)
    return a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])


def refused(lay, rows, cols, channels=1, frames=1):
    """check_plane's layout rules (wm_api.hip) restated: rows inside the pitch, channel planes and frames that do not overlap"""
    if lay.pitch < cols:
        return True
    if channels > 1 and lay.channel_stride < rows * lay.pitch:
        return True
    if frames > 1 and lay.frame_stride < (channels - 1) * (lay.channel_stride if channels > 1 else 0) + rows * lay.pitch:
        return True
    return False


def vector_path(lay, itemsize, channels=1, frames=1):
    """wm.h's rule for the kernels' vector path on a buffer whose own base is aligned: f32 planes need a 4-byte aligned base (always
    true of an element offset); u8 planes need base, pitch and the strides in use to be multiples of 4 bytes"""
    if itemsize == 4:
        return True
    if lay.offset % 4 or lay.pitch % 4:
        return False
    if frames > 1 and lay.frame_stride % 4:
        return False
    if channels > 1 and lay.channel_stride % 4:
        return False
    return True
