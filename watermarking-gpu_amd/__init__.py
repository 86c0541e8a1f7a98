"""MI355X-native watermark engine: Python host-side mirror of the reference's `Watermark` class.

The reference is C++ (Watermark_GPU/Watermark.hpp:26-72); its C++ drop-in is include/Watermark.hpp.
This module is the same surface for Python callers (tests, bench.py): same class and method names,
argument order and error behaviour, over the C ABI of include/wm.h loaded with ctypes.  Arrays are
torch CUDA tensors (torch is plumbing here: device memory, streams, torch.distributed) standing in
for af::array: [rows, cols] grey, [3, rows, cols] planar RGB, or a batch [frames, rows, cols].

There is NO CPU fallback: without libwm_hip.so or without a HIP device every operation raises.
"""
import ctypes as C
import enum
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libwm_hip.so")

WM_OK, WM_UNSOLVABLE = 0, 1
WM_ERR_BAD_P, WM_ERR_W_OPEN, WM_ERR_W_SIZE, WM_ERR_RUNTIME = -1, -2, -3, -4
WM_ERR_BAD_ARG, WM_ERR_NO_DEVICE, WM_ERR_ALLOC, WM_ERR_PSNR, WM_ERR_BUSY = -5, -6, -7, -8, -9
WM_SLOT_SYNC = -1
WM_F32, WM_U8, WM_U16 = 0, 1, 2
WM_MEM_DEVICE, WM_MEM_HOST, WM_MEM_SLOT_OUT = 0, 1, 2
WM_KEYS_MAX = 4096


class MASK_TYPE(enum.IntEnum):
    """Watermark.hpp:10-14"""
    ME = 0
    NVF = 1


class wm_plane(C.Structure):
    _fields_ = [("data", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32), ("channels", C.c_int32),
                ("dtype", C.c_int32), ("mem", C.c_int32), ("frames", C.c_int32), ("pitch", C.c_int64),
                ("channel_stride", C.c_int64), ("frame_stride", C.c_int64)]


class wm_packed(C.Structure):
    """interleaved 8-bit R, G, B pixels (wm.h wm_packed); strides in bytes"""
    _fields_ = [("data", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32), ("mem", C.c_int32), ("frames", C.c_int32),
                ("pitch_bytes", C.c_int64), ("frame_stride_bytes", C.c_int64)]


# every symbol include/wm.h declares: (name, restype, argtypes)
_P = C.POINTER
_ctx_p = C.c_void_p
ABI = [
    ("wm_create", C.c_int, [_P(_ctx_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P(C.c_float)]),
    ("wm_create_from_file", C.c_int, [_P(_ctx_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_char_p]),
    ("wm_create_generated", C.c_int, [_P(_ctx_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint32]),
    ("wm_clone", C.c_int, [_ctx_p, _P(_ctx_p)]),
    ("wm_reinit", C.c_int, [_ctx_p, C.c_int, C.c_int, _P(C.c_float)]),
    ("wm_reinit_from_file", C.c_int, [_ctx_p, C.c_int, C.c_int, C.c_char_p]),
    ("wm_destroy", None, [_ctx_p]),
    ("wm_configure", C.c_int, [_ctx_p, C.c_int, C.c_int]),
    ("wm_set_fused", C.c_int, [_ctx_p, C.c_int]),
    ("wm_set_handover", C.c_int, [_ctx_p, C.c_int]),
    ("wm_set_checked_handover", C.c_int, [_ctx_p, C.c_int]),
    ("wm_checked_handover_counts", C.c_int, [_ctx_p, _P(C.c_ulonglong), _P(C.c_ulonglong)]),
    ("wm_fused_info", C.c_int, [_ctx_p, _P(C.c_int), _P(C.c_int), _P(C.c_ulonglong)]),
    ("wm_fused_lock_skips", C.c_ulonglong, [_ctx_p]),
    ("wm_fused_stamps", C.c_int, [_ctx_p, _P(C.c_ulonglong), C.c_int]),
    ("wm_fused_gram", C.c_int, [_ctx_p, _P(C.c_double)]),
    ("wm_selftest_nvf_quotient", C.c_int, [C.c_int, C.c_int, C.c_uint32, C.c_uint32, _P(C.c_ulonglong), _P(C.c_uint32)]),
    ("wm_set_rows_per_segment", C.c_int, [_ctx_p, C.c_int]),
    ("wm_embed", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), _P(wm_plane), _P(wm_plane), _P(C.c_float), _P(C.c_int), C.c_int]),
    ("wm_detect", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), _P(C.c_float), _P(C.c_int), C.c_int]),
    ("wm_embed_detect", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), _P(wm_plane), _P(wm_plane), _P(C.c_float), _P(C.c_float), _P(C.c_int), C.c_int]),
    ("wm_keys_create", C.c_int, [_P(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int]),
    ("wm_keys_destroy", None, [C.c_void_p]),
    ("wm_keys_count", C.c_int, [C.c_void_p]),
    ("wm_keys_rows", C.c_int, [C.c_void_p]),
    ("wm_keys_cols", C.c_int, [C.c_void_p]),
    ("wm_keys_device_ptr", C.c_void_p, [C.c_void_p, C.c_int]),
    ("wm_keys_set", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    ("wm_keys_load_file", C.c_int, [C.c_void_p, C.c_int, C.c_char_p]),
    ("wm_keys_generate", C.c_int, [C.c_void_p, C.c_int, C.c_uint32]),
    ("wm_detect_keys", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), C.c_void_p, _P(C.c_float), _P(C.c_int), C.c_int]),
    ("wm_embed_keys", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), _P(wm_plane), C.c_void_p, _P(wm_plane), _P(C.c_float), _P(C.c_int), C.c_int]),
    ("wm_offsets_check", C.c_int, [C.c_int] * 8),
    ("wm_detect_offsets_group", C.c_int, []),
    ("wm_detect_offsets", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_float), _P(C.c_int),
                                   C.c_int]),
    ("wm_locate_shape", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_int), _P(C.c_int), _P(C.c_int), _P(C.c_int)]),
    ("wm_locate", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), C.c_void_p, C.c_int, _P(C.c_float), C.c_void_p, _P(C.c_int), C.c_int]),
    ("wm_locate_bits", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, _P(C.c_float),
                                 _P(C.c_float), C.c_void_p, C.c_void_p, _P(C.c_int), C.c_int]),
    ("wm_locate_bits_cover", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, _P(C.c_int64)]),
    ("wm_locate_bits_bench", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_double)]),
    ("wm_locate_keys", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), C.c_void_p, C.c_int, C.c_int, _P(C.c_float), C.c_void_p, _P(C.c_int), C.c_int]),
    ("wm_locate_keys_rank", C.c_int, [_P(C.c_float), C.c_int, _P(C.c_int), _P(C.c_float), _P(C.c_float)]),
    ("wm_locate_keys_bench", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_double)]),
    ("wm_clip_pool", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), _P(C.c_float), C.c_void_p, C.c_int, _P(C.c_int), C.c_int]),
    ("wm_locate_pooled", C.c_int, [_ctx_p, C.c_void_p, C.c_void_p, C.c_int, _P(C.c_float), C.c_void_p, C.c_int]),
    ("wm_locate_bits_pooled", C.c_int, [_ctx_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, _P(C.c_float), _P(C.c_float),
                                        C.c_void_p, C.c_void_p, C.c_int]),
    ("wm_locate_keys_pooled", C.c_int, [_ctx_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, _P(C.c_float), C.c_void_p, C.c_int]),
    ("wm_clip_pool_bench", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_double), _P(C.c_int)]),
    ("wm_fft2", C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    ("wm_fft_bench", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_double)]),
    ("wm_tiles_shape", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_int), _P(C.c_int)]),
    ("wm_detect_tiles", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), C.c_int, C.c_int, C.c_void_p, C.c_void_p, _P(C.c_int), C.c_int]),
    ("wm_detect_keys_tiles", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, _P(C.c_int), C.c_int]),
    ("wm_bits_layout", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_uint64, _P(C.c_int32)]),
    ("wm_embed_signs", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), _P(wm_plane), _P(wm_plane), C.c_int, C.c_int, C.c_void_p, _P(C.c_float), _P(C.c_int),
                                C.c_int]),
    ("wm_embed_bits", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), _P(wm_plane), _P(wm_plane), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                               _P(C.c_float), _P(C.c_int), C.c_int]),
    ("wm_detect_bits", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), C.c_int, C.c_int, C.c_void_p, C.c_int, _P(C.c_float), _P(C.c_int), C.c_int]),
    ("wm_embed_signs_group", C.c_int, []),
    ("wm_embed_signs_multi", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), _P(wm_plane), _P(wm_plane), C.c_int, C.c_int, C.c_int, C.c_void_p, _P(C.c_float),
                                      _P(C.c_int), C.c_int]),
    ("wm_embed_bits_multi", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), _P(wm_plane), _P(wm_plane), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                     C.c_void_p, _P(C.c_float), _P(C.c_int), C.c_int]),
    ("wm_key_schedule", C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.c_int, _P(C.c_int32)]),
    ("wm_embed_select", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), _P(wm_plane), _P(wm_plane), C.c_void_p, _P(C.c_int32), _P(C.c_float), _P(C.c_int),
                                 C.c_int]),
    ("wm_detect_select", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), C.c_void_p, _P(C.c_int32), _P(C.c_float), _P(C.c_int), C.c_int]),
    ("wm_rgb2gray", C.c_int, [_ctx_p, _P(wm_plane), _P(wm_plane), _P(C.c_float), C.c_int]),
    ("wm_unpack_rgb8", C.c_int, [_ctx_p, _P(wm_packed), _P(wm_plane), _P(wm_plane), _P(C.c_float), C.c_int]),
    ("wm_pack_rgb8", C.c_int, [_ctx_p, _P(wm_plane), _P(wm_packed), C.c_int]),
    ("wm_depth_scale", C.c_int, [C.c_int, _P(C.c_float), _P(C.c_float)]),
    ("wm_unpack16", C.c_int, [_ctx_p, _P(wm_plane), C.c_int, C.c_int, _P(wm_plane), C.c_int]),
    ("wm_pack16", C.c_int, [_ctx_p, _P(wm_plane), _P(wm_plane), C.c_int, C.c_int, C.c_int]),
    ("wm_embed16", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), _P(wm_plane), C.c_int, C.c_int, _P(C.c_float), _P(C.c_int), C.c_int]),
    ("wm_detect16", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), C.c_int, C.c_int, _P(C.c_float), _P(C.c_int), C.c_int]),
    ("wm_quality", C.c_int, [_ctx_p, _P(wm_plane), _P(wm_plane), C.c_int, C.c_int, _P(C.c_float), C.c_void_p, C.c_int]),
    ("wm_psnr_from_mse", C.c_double, [C.c_double, C.c_double]),
    ("wm_compute_mask", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), _P(wm_plane), _P(wm_plane), _P(C.c_float), _P(C.c_int), C.c_int]),
    ("wm_gram", C.c_int, [_ctx_p, _P(wm_plane), _P(C.c_double), C.c_int]),
    ("wm_band_configure", C.c_int, [_ctx_p, C.c_int, C.c_int, C.c_longlong]),
    ("wm_band_solve", C.c_int, [_ctx_p, _P(C.c_double), C.c_int, _P(C.c_int), C.c_int]),
    ("wm_band_stats", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), _P(C.c_double), C.c_int]),
    ("wm_band_embed", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), _P(wm_plane), _P(wm_plane), _P(C.c_double), _P(C.c_float), C.c_int]),
    ("wm_band_detect_sums", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), _P(C.c_double), C.c_int]),
    ("wm_band_gram_dev", C.c_int, [_ctx_p, _P(wm_plane), C.c_void_p, C.c_int]),
    ("wm_band_solve_dev", C.c_int, [_ctx_p, C.c_void_p, C.c_int, C.c_int]),
    ("wm_band_stats_dev", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), C.c_void_p, C.c_int]),
    ("wm_band_embed_dev", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), _P(wm_plane), _P(wm_plane), C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    ("wm_band_detect_sums_dev", C.c_int, [_ctx_p, C.c_int, _P(wm_plane), C.c_void_p, C.c_int]),
    ("wm_band_corr_dev", C.c_int, [_ctx_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    ("wm_sync", C.c_int, [_ctx_p, C.c_int]),
    ("wm_set_stream", C.c_int, [_ctx_p, C.c_int, C.c_void_p]),
    ("wm_get_stream", C.c_void_p, [_ctx_p, C.c_int]),
    ("wm_dev_alloc", C.c_void_p, [C.c_int, C.c_size_t]),
    ("wm_dev_free", None, [C.c_void_p]),
    ("wm_memcpy_h2d", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("wm_memcpy_d2h", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("wm_device_count", C.c_int, []),
    ("wm_host_alloc", C.c_void_p, [C.c_size_t]),
    ("wm_host_free", None, [C.c_void_p]),
    ("wm_membench", C.c_int, [C.c_int, C.c_int, C.c_size_t, C.c_double, _P(C.c_double), _P(C.c_int)]),
    ("wm_rows", C.c_int, [_ctx_p]),
    ("wm_cols", C.c_int, [_ctx_p]),
    ("wm_p", C.c_int, [_ctx_p]),
    ("wm_strength_factor", C.c_float, [_ctx_p]),
    ("wm_device", C.c_int, [_ctx_p]),
    ("wm_w_device", C.c_void_p, [_ctx_p]),
    ("wm_prof_enable", C.c_int, [_ctx_p, C.c_int]),
    ("wm_prof_reset", C.c_int, [_ctx_p]),
    ("wm_prof_kernel_count", C.c_int, []),
    ("wm_prof_kernel_name", C.c_char_p, [C.c_int]),
    ("wm_prof_get", C.c_int, [_ctx_p, C.c_int, _P(C.c_uint64), _P(C.c_double)]),
    ("wm_strerror", C.c_char_p, [C.c_int]),
    ("wm_last_error", C.c_char_p, [_ctx_p]),
    ("wm_version", C.c_char_p, []),
]

_lib = None


def lib():
    """loads libwm_hip.so; raises (loudly) if the HIP extension has not been built"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(make -C watermarking-gpu_amd/csrc).  There is no CPU fallback.")
        # one HIP runtime per process: PyTorch ships its own libamdhip64 and this module hands torch tensors to the
        # library, so torch's runtime has to be the one libwm_hip.so binds to -- load torch first, whatever the
        # import order of the caller (a second runtime loaded afterwards sees no device)
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, res, args in ABI:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def strerror(code):
    return lib().wm_strerror(code).decode()


def _raise(code, ctx=None):
    detail = ""
    if ctx:
        detail = lib().wm_last_error(ctx).decode()
    msg = strerror(code) + (": " + detail if detail else "")
    # the reference throws std::runtime_error for all of these (Watermark.cpp:24-25,65-66,70-71,111-113)
    raise RuntimeError(msg)


def plane_of(t, channels=1, batched=None):
    """wm_plane view of a torch CUDA tensor: [R,C], [3,R,C] (channels=3) or [F,R,C] / [F,3,R,C]"""
    import torch
    if not t.is_cuda:
        raise RuntimeError("plane tensors must live on the GPU (no CPU fallback)")
    if t.dtype == torch.float32:
        dt = WM_F32
    elif t.dtype == torch.uint8:
        dt = WM_U8
    else:
        raise RuntimeError(f"unsupported dtype {t.dtype}")
    if t.stride(-1) != 1:
        raise RuntimeError("innermost stride must be 1 (row-major planes)")
    nd = t.dim()
    base_nd = 2 if channels == 1 else 3
    if nd == base_nd:
        frames, fstride = 1, 0
    elif nd == base_nd + 1:
        frames, fstride = t.shape[0], t.stride(0)
    else:
        raise RuntimeError(f"bad tensor rank {nd} for channels={channels}")
    cstride = t.stride(-3) if channels > 1 else 0
    if channels > 1 and t.shape[-3] != channels:
        raise RuntimeError("channel dimension mismatch")
    return wm_plane(t.data_ptr(), t.shape[-2], t.shape[-1], channels, dt, WM_MEM_DEVICE, frames, t.stride(-2), cstride,
                    fstride)


def packed_of(t):
    """wm_packed view of a uint8 torch tensor of interleaved pixels: [R, C, 3] or a batch [F, R, C, 3] whose pixels are three
    adjacent bytes (rows and frames may be padded).  A GPU tensor is a device buffer, a CPU tensor a WM_MEM_HOST one (it must stay
    alive until the slot is synced)"""
    import torch
    if t.dtype != torch.uint8:
        raise RuntimeError(f"packed pixels must be uint8, got {t.dtype}")
    if t.dim() not in (3, 4) or t.shape[-1] != 3 or t.stride(-1) != 1 or t.stride(-2) != 3:
        raise RuntimeError("packed pixels must be [R, C, 3] or [F, R, C, 3] with three adjacent bytes per pixel")
    frames, fstride = (t.shape[0], t.stride(0)) if t.dim() == 4 else (1, 0)
    return wm_packed(t.data_ptr(), t.shape[-3], t.shape[-2], WM_MEM_DEVICE if t.is_cuda else WM_MEM_HOST, frames, t.stride(-3), fstride)


def depth_scale(bits):
    """(k_in, k_out) of wm.h wm_depth_scale: the f32 constants that take a `bits`-bit sample to [0, 255] and back"""
    a, b = C.c_float(), C.c_float()
    rc = lib().wm_depth_scale(int(bits), C.byref(a), C.byref(b))
    if rc != WM_OK:
        _raise(rc)
    return a.value, b.value


def plane_any(t, channels=1):
    """wm_plane view of a row-major array for the 16-bit calls (wm.h wm_unpack16 ...): [R,C], [3,R,C] (channels=3) or a batch of
    either.  A numpy array or a CPU torch tensor is a WM_MEM_HOST plane (it must stay alive until the slot is synced), a GPU torch
    tensor a device plane.  float32 is WM_F32; numpy uint16 and torch uint16 / int16 (the 16-bit pattern is the sample) are WM_U16"""
    import numpy as np
    if isinstance(t, np.ndarray):
        if t.dtype not in (np.float32, np.uint16) or any(st % t.itemsize for st in t.strides):
            raise RuntimeError(f"unsupported numpy array {t.dtype} / strides {t.strides}")
        dt = WM_F32 if t.dtype == np.float32 else WM_U16
        shape, strides, ptr, mem = t.shape, [st // t.itemsize for st in t.strides], t.ctypes.data, WM_MEM_HOST
    else:
        import torch
        if t.dtype == torch.float32:
            dt = WM_F32
        elif t.dtype in (torch.int16, getattr(torch, "uint16", torch.int16)):
            dt = WM_U16
        else:
            raise RuntimeError(f"unsupported dtype {t.dtype}")
        shape, strides, ptr, mem = tuple(t.shape), list(t.stride()), t.data_ptr(), WM_MEM_DEVICE if t.is_cuda else WM_MEM_HOST
    nd, base_nd = len(shape), 2 if channels == 1 else 3
    if nd not in (base_nd, base_nd + 1) or strides[-1] != 1 or (channels > 1 and shape[-3] != channels):
        raise RuntimeError(f"bad shape {tuple(shape)} / strides {tuple(strides)} for channels={channels}")
    frames, fstride = (shape[0], strides[0]) if nd == base_nd + 1 else (1, 0)
    return wm_plane(ptr, shape[-2], shape[-1], channels, dt, mem, frames, strides[-2], strides[-3] if channels > 1 else 0, fstride)


WM_QUALITY_NVALS, WM_QUALITY_NSUMS = 3, 5
WM_LOCATE_NVALS = 4


def locate_shape(rows, cols, key_rows, key_cols):
    """(ny, nx, pr, pc) of wm_locate_shape: the admissible offsets per axis of a rows x cols image in a key_rows x key_cols key plane and
    the padded power-of-two transform.  Raises for a key smaller than the image or a transform above 8192 per axis"""
    v = [C.c_int() for _ in range(4)]
    rc = lib().wm_locate_shape(rows, cols, key_rows, key_cols, *[C.byref(x) for x in v])
    if rc != WM_OK:
        _raise(rc)
    return tuple(x.value for x in v)


WM_LOCATE_BITS_NVALS = 4


def locate_bits_cover(rows, cols, key_rows, key_cols, tile_rows, tile_cols, tile_bit, nbits, oy, ox):
    """wm.h wm_locate_bits_cover: an int64 numpy array [nbits], the pixels of the rows x cols window at (oy, ox) of the key plane whose
    key tile carries bit b (tile_bit: int32 [ty * tx] over the KEY plane).  Raises for what the library refuses"""
    tb = np.ascontiguousarray(tile_bit, np.int32).reshape(-1)
    px = np.zeros(max(nbits, 1), np.int64)
    ny, nx = C.c_int(), C.c_int()
    if lib().wm_tiles_shape(key_rows, key_cols, tile_rows, tile_cols, C.byref(ny), C.byref(nx)) != WM_OK or tb.size != ny.value * nx.value:
        raise RuntimeError("locate_bits_cover: bad tile shape, or tile_bit is not the table of the key plane's tiles")
    rc = lib().wm_locate_bits_cover(rows, cols, key_rows, key_cols, tile_rows, tile_cols, tb.ctypes.data_as(C.c_void_p), nbits, oy, ox,
                                    px.ctypes.data_as(_P(C.c_int64)))
    if rc != WM_OK:
        _raise(rc)
    return px[:nbits]


FFT_BENCH_PASSES = ("rows_pc", "transpose", "rows_pr", "product", "rows_pr_inverse", "transpose_back", "rows_pc_inverse")


def fft_bench(pr, pc, iters=20, device=0):
    """wm.h wm_fft_bench: {pass: mean microseconds per launch} of the seven passes one frame of wm_locate makes over a pr x pc plane"""
    us = (C.c_double * len(FFT_BENCH_PASSES))()
    rc = lib().wm_fft_bench(device, pr, pc, iters, us)
    if rc != WM_OK:
        _raise(rc)
    return dict(zip(FFT_BENCH_PASSES, us))


LOCATE_BITS_BENCH_PASSES = ("key_pair", "product3", "accumulate")


def locate_bits_bench(pr, pc, ny, nx, iters=20, device=0):
    """wm.h wm_locate_bits_bench: {pass: mean microseconds per launch} of the three passes wm_locate_bits adds to a transform's seven"""
    us = (C.c_double * len(LOCATE_BITS_BENCH_PASSES))()
    rc = lib().wm_locate_bits_bench(device, pr, pc, ny, nx, iters, us)
    if rc != WM_OK:
        _raise(rc)
    return dict(zip(LOCATE_BITS_BENCH_PASSES, us))


WM_LOCATE_KEYS_NVALS = 4
LOCATE_KEYS_BENCH_PASSES = ("keys_pair", "keys_peak")


def clip_pool_bench(rows, cols, frames, mask=0, p=3, iters=20, device=0):
    """wm.h wm_clip_pool_bench: ({"lds_tile": us, "gather": us} per launch of the pool kernel's two routes, whether their pools have
    equal bits)"""
    us, eq = (C.c_double * 2)(), C.c_int()
    rc = lib().wm_clip_pool_bench(device, rows, cols, frames, int(mask), p, iters, us, C.byref(eq))
    if rc != WM_OK:
        _raise(rc)
    return {"lds_tile": us[0], "gather": us[1]}, bool(eq.value)


def locate_keys_rank(loc):
    """wm.h wm_locate_keys_rank on one frame's records [nk, 4] of Watermark.locateKeys: (best, z_best, z_next) -- the index of the key
    with the largest z (NaN is ignored, ties: the smallest index; -1 when every z is NaN), that z, and the largest z among the others
    (NaN when there is none)"""
    a = np.ascontiguousarray(loc, np.float32)
    if a.ndim != 2 or a.shape[1] != WM_LOCATE_KEYS_NVALS:
        raise RuntimeError("locate_keys_rank: loc must be one frame's [nk, 4] records")
    best, zb, zn = C.c_int(), C.c_float(), C.c_float()
    rc = lib().wm_locate_keys_rank(a.ctypes.data_as(_P(C.c_float)), a.shape[0], C.byref(best), C.byref(zb), C.byref(zn))
    if rc != WM_OK:
        _raise(rc)
    return best.value, zb.value, zn.value


def locate_keys_bench(pr, pc, ny, nx, iters=20, device=0):
    """wm.h wm_locate_keys_bench: {pass: mean microseconds per launch} of the two passes wm_locate_keys adds to a transform's seven
    and wm_locate_bits_bench's product"""
    us = (C.c_double * len(LOCATE_KEYS_BENCH_PASSES))()
    rc = lib().wm_locate_keys_bench(device, pr, pc, ny, nx, iters, us)
    if rc != WM_OK:
        _raise(rc)
    return dict(zip(LOCATE_KEYS_BENCH_PASSES, us))


def fft2(t, inverse=False):
    """wm.h wm_fft2, a building block for parity tests: the 2-D transform of a contiguous float32 GPU tensor [pr, pc, 2] (interleaved
    complex) IN PLACE, exp(-2 pi i ..) forward, exp(+2 pi i ..) inverse, neither normalised; pr, pc powers of two in 64 .. 8192"""
    import torch
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 3 and t.shape[2] == 2):
        raise RuntimeError("fft2 takes a contiguous float32 GPU tensor [pr, pc, 2]")
    torch.cuda.current_stream().synchronize()
    rc = lib().wm_fft2(t.device.index or 0, C.c_void_p(t.data_ptr()), t.shape[0], t.shape[1], 1 if inverse else 0)
    if rc != WM_OK:
        _raise(rc)
    return t


def psnr_from_mse(mse, peak=255.0):
    """wm.h wm_psnr_from_mse: 10 log10(peak^2 / mse); +inf for mse == 0, NaN for a negative or NaN mse or peak <= 0"""
    return lib().wm_psnr_from_mse(float(mse), float(peak))


def plane_u8f32(t, channels=1):
    """wm_plane view of a float32 or uint8 row-major array for wm_quality: [R,C], [3,R,C] (channels=3) or a batch of either.  A GPU
    torch tensor is a device plane (plane_of); a numpy array or a CPU torch tensor is a WM_MEM_HOST plane (it must stay alive until
    the slot is synced)"""
    if isinstance(t, np.ndarray):
        if t.dtype not in (np.float32, np.uint8) or any(st % t.itemsize for st in t.strides):
            raise RuntimeError(f"unsupported numpy array {t.dtype} / strides {t.strides}")
        dt = WM_F32 if t.dtype == np.float32 else WM_U8
        shape, strides, ptr = t.shape, [st // t.itemsize for st in t.strides], t.ctypes.data
    else:
        import torch
        if t.is_cuda:
            return plane_of(t, channels)
        if t.dtype not in (torch.float32, torch.uint8):
            raise RuntimeError(f"unsupported dtype {t.dtype}")
        dt = WM_F32 if t.dtype == torch.float32 else WM_U8
        shape, strides, ptr = tuple(t.shape), list(t.stride()), t.data_ptr()
    nd, base_nd = len(shape), 2 if channels == 1 else 3
    if nd not in (base_nd, base_nd + 1) or strides[-1] != 1 or (channels > 1 and shape[-3] != channels):
        raise RuntimeError(f"bad shape {tuple(shape)} / strides {tuple(strides)} for channels={channels}")
    frames, fstride = (shape[0], strides[0]) if nd == base_nd + 1 else (1, 0)
    return wm_plane(ptr, shape[-2], shape[-1], channels, dt, WM_MEM_HOST, frames, strides[-2], strides[-3] if channels > 1 else 0, fstride)


class KeySet:
    """A bank of watermark keys on one device (wm.h wm_keys_*): K planes [rows, cols] f32 that Watermark.detectKeys scores an
    image against in one call.  The bank owns copies of its planes."""

    def __init__(self, rows, cols, nkeys, device=0):
        self._keys = C.c_void_p()
        rc = lib().wm_keys_create(C.byref(self._keys), device, rows, cols, nkeys)
        if rc != WM_OK:
            self._keys = C.c_void_p()
            _raise(rc)

    @classmethod
    def from_seeds(cls, rows, cols, seeds, device=0):
        """key k = the W of Watermark.generated(rows, cols, seeds[k], ...) (wm_keys_generate)"""
        seeds = list(seeds)
        self = cls(rows, cols, len(seeds), device)
        for k, sd in enumerate(seeds):
            self._chk(lib().wm_keys_generate(self._keys, k, int(sd) & 0xFFFFFFFF))
        return self

    @classmethod
    def from_files(cls, paths, rows, cols, device=0):
        """key k = the raw f32 W file paths[k] (wm_keys_load_file)"""
        paths = list(paths)
        self = cls(rows, cols, len(paths), device)
        for k, p in enumerate(paths):
            self._chk(lib().wm_keys_load_file(self._keys, k, os.fsencode(p)))
        return self

    def _chk(self, rc):
        if rc != WM_OK:
            self.close()
            _raise(rc)

    def set(self, k, w):
        """key k := a [rows, cols] float32 torch tensor (on the GPU or not) or numpy array"""
        if isinstance(w, np.ndarray):
            a = np.ascontiguousarray(w, dtype=np.float32)
            if a.size != self.rows * self.cols:
                _raise(WM_ERR_BAD_ARG)
            rc = lib().wm_keys_set(self._keys, k, a.ctypes.data_as(C.c_void_p), WM_MEM_HOST)
        else:
            import torch
            t = w.detach().to(torch.float32).contiguous()
            if t.numel() != self.rows * self.cols:
                _raise(WM_ERR_BAD_ARG)
            if t.is_cuda:
                torch.cuda.current_stream().synchronize()
            rc = lib().wm_keys_set(self._keys, k, C.c_void_p(t.data_ptr()), WM_MEM_DEVICE if t.is_cuda else WM_MEM_HOST)
        if rc != WM_OK:
            _raise(rc)

    def plane(self, k):
        """key k as a numpy array [rows, cols] (downloaded)"""
        w = np.empty((self.rows, self.cols), np.float32)
        p = lib().wm_keys_device_ptr(self._keys, k)
        if not p:
            _raise(WM_ERR_BAD_ARG)
        rc = lib().wm_memcpy_d2h(w.ctypes.data_as(C.c_void_p), p, w.nbytes)
        if rc != WM_OK:
            _raise(rc)
        return w

    @property
    def handle(self):
        return self._keys

    @property
    def count(self):
        return lib().wm_keys_count(self._keys)

    def __len__(self):
        return self.count

    @property
    def rows(self):
        return lib().wm_keys_rows(self._keys)

    @property
    def cols(self):
        return lib().wm_keys_cols(self._keys)

    def close(self):
        if getattr(self, "_keys", None):
            lib().wm_keys_destroy(self._keys)
            self._keys = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _keys_handle(keys):
    """a KeySet or a raw wm_keys handle"""
    return keys.handle if isinstance(keys, KeySet) else keys


class Watermark:
    """Functions for watermark computation and detection (Watermark.hpp:26-72).

    Watermark(rows, cols, randomMatrixPath, p, psnr): `randomMatrixPath` is the raw f32 W file
    (Watermark.cpp:62-75) or a numpy array [rows, cols].  The reference's `programs` argument
    (pre-built OpenCL programs) has no counterpart: kernels are compiled into libwm_hip.so.
    """

    def __init__(self, rows, cols, randomMatrixPath, p, psnr, device=0, nslots=2, max_frames=1):
        L = lib()
        self._ctx = _ctx_p()
        if isinstance(randomMatrixPath, (str, bytes, os.PathLike)):
            rc = L.wm_create_from_file(C.byref(self._ctx), device, rows, cols, p, psnr, os.fsencode(randomMatrixPath))
        else:
            w = np.ascontiguousarray(randomMatrixPath, dtype=np.float32)
            if w.size != rows * cols:
                _raise(WM_ERR_W_SIZE)
            rc = L.wm_create(C.byref(self._ctx), device, rows, cols, p, psnr, w.ctypes.data_as(_P(C.c_float)))
        if rc != WM_OK:
            self._ctx = _ctx_p()
            _raise(rc)
        self._max_frames = 1  # (wm_create's; configure keeps it current: what locateClip cuts a clip by)
        if (nslots, max_frames) != (2, 1):
            self.configure(nslots, max_frames)

    def _chk(self, rc):
        """a call's return code: raises for an error (negative), passes WM_OK / WM_UNSOLVABLE on"""
        if rc < 0:
            _raise(rc, self._ctx)
        return rc

    @classmethod
    def generated(cls, rows, cols, seed, p, psnr, device=0, nslots=2, max_frames=1):
        """an engine whose W is generated on the device from `seed` (wm.h wm_create_generated; the matrix wm_genw writes)"""
        self = object.__new__(cls)
        self._ctx = _ctx_p()
        rc = lib().wm_create_generated(C.byref(self._ctx), device, rows, cols, p, psnr, seed & 0xFFFFFFFF)
        if rc != WM_OK:
            self._ctx = _ctx_p()
            _raise(rc)
        self._max_frames = 1  # (wm_create's; configure keeps it current: what locateClip cuts a clip by)
        if (nslots, max_frames) != (2, 1):
            self.configure(nslots, max_frames)
        return self

    def watermark(self):
        """the engine's W as a numpy array [rows, cols] (downloaded)"""
        w = np.empty((self.rows, self.cols), np.float32)
        rc = lib().wm_memcpy_d2h(w.ctypes.data_as(C.c_void_p), lib().wm_w_device(self._ctx), w.nbytes)
        if rc != WM_OK:
            _raise(rc, self._ctx)
        return w

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            lib().wm_destroy(self._ctx)
            self._ctx = _ctx_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def copy(self):
        """copy constructor (Watermark.cpp:30-37): shares W, owns new scratch"""
        other = object.__new__(Watermark)
        other._ctx = _ctx_p()
        rc = lib().wm_clone(self._ctx, C.byref(other._ctx))
        if rc != WM_OK:
            _raise(rc, self._ctx)
        other._max_frames = self._max_frames  # (wm_clone carries the configuration over)
        return other

    def reinitialize(self, randomMatrixPath, rows, cols):
        """Watermark.cpp:78-85"""
        if isinstance(randomMatrixPath, (str, bytes, os.PathLike)):
            rc = lib().wm_reinit_from_file(self._ctx, rows, cols, os.fsencode(randomMatrixPath))
        else:
            w = np.ascontiguousarray(randomMatrixPath, dtype=np.float32)
            if w.size != rows * cols:
                _raise(WM_ERR_W_SIZE)
            rc = lib().wm_reinit(self._ctx, rows, cols, w.ctypes.data_as(_P(C.c_float)))
        if rc != WM_OK:
            _raise(rc, self._ctx)

    def configure(self, nslots, max_frames):
        rc = lib().wm_configure(self._ctx, nslots, max_frames)
        if rc != WM_OK:
            _raise(rc, self._ctx)
        self._max_frames = max_frames

    def set_fused(self, on):
        """one-frame synchronous calls as ONE launch with LDS-resident tiles (wm.h wm_set_fused); on by default"""
        rc = lib().wm_set_fused(self._ctx, 1 if on else 0)
        if rc != WM_OK:
            _raise(rc, self._ctx)

    def set_handover(self, on):
        """Gram hand-over from embed to a detector reading WM_MEM_SLOT_OUT (wm.h wm_set_handover); off by default"""
        rc = lib().wm_set_handover(self._ctx, 1 if on else 0)
        if rc != WM_OK:
            _raise(rc, self._ctx)

    def set_checked_handover(self, on):
        """wm_detect of the plane the slot's last embed wrote, checked by a digest of it (wm.h wm_set_checked_handover); on by default"""
        rc = lib().wm_set_checked_handover(self._ctx, 1 if on else 0)
        if rc != WM_OK:
            _raise(rc, self._ctx)

    def checked_handover_counts(self):
        """(trusted, redone): frames of checked hand-overs since the context was configured (wm.h wm_checked_handover_counts)"""
        t, r = C.c_ulonglong(0), C.c_ulonglong(0)
        rc = lib().wm_checked_handover_counts(self._ctx, C.byref(t), C.byref(r))
        if rc != WM_OK:
            _raise(rc, self._ctx)
        return t.value, r.value

    def fused_info(self):
        """(active, workgroups, tile_rows, fallbacks)"""
        g, th, fb = C.c_int(), C.c_int(), C.c_ulonglong()
        act = lib().wm_fused_info(self._ctx, C.byref(g), C.byref(th), C.byref(fb))
        return bool(act), g.value, th.value, fb.value

    def set_rows_per_segment(self, rps):
        rc = lib().wm_set_rows_per_segment(self._ctx, rps)
        if rc != WM_OK:
            _raise(rc, self._ctx)

    # -- properties -------------------------------------------------------------------------
    @property
    def rows(self):
        return lib().wm_rows(self._ctx)

    @property
    def cols(self):
        return lib().wm_cols(self._ctx)

    @property
    def strengthFactor(self):
        return lib().wm_strength_factor(self._ctx)

    # -- the hot path -------------------------------------------------------------------------
    def makeWatermark(self, inputImage, outputImage, maskType, out=None):
        """Watermark.cpp:156-172.  inputImage: grey [R,C] (or batch [F,R,C]); outputImage: the base the
        watermark is added to ([R,C], [3,R,C] or batched).  Returns (watermarked, watermarkStrength);
        the reference returns the array and writes the strength through a float& argument.
        Unsolvable system: returns outputImage unchanged and strength None (reference leaves it unset)."""
        import torch
        if out is None:
            out = torch.empty_like(outputImage)
        pin, pbase, pout = self._embed_planes(inputImage, outputImage, out)
        a, st = self._strength_bufs(pin.frames)
        torch.cuda.current_stream().synchronize()
        self._chk(lib().wm_embed(self._ctx, int(maskType), C.byref(pin), C.byref(pbase), C.byref(pout), a, st, WM_SLOT_SYNC))
        return out, self._strengths(a, st, inputImage.dim() == 2)

    def detectWatermark(self, watermarkedImage, maskType):
        """Watermark.cpp:234-250; 0.0 for an unsolvable system"""
        import torch
        pimg = plane_of(watermarkedImage, 1)
        frames = pimg.frames
        corr = (C.c_float * frames)()
        torch.cuda.current_stream().synchronize()
        self._chk(lib().wm_detect(self._ctx, int(maskType), C.byref(pimg), corr, None, WM_SLOT_SYNC))
        if watermarkedImage.dim() == 2:
            return corr[0]
        return list(corr)

    def detectKeys(self, image, keys, maskType):
        """detectWatermark of `image` against every key of the KeySet `keys` in one call (wm.h wm_detect_keys): a float32 numpy
        array [frames, K] ([K] for one grey frame); 0.0 for every key of an unsolvable frame"""
        import torch
        pimg = plane_of(image, 1)
        frames, K = pimg.frames, keys.count
        corr = np.zeros((frames, K), np.float32)
        torch.cuda.current_stream().synchronize()
        self._chk(lib().wm_detect_keys(self._ctx, int(maskType), C.byref(pimg), keys.handle, corr.ctypes.data_as(_P(C.c_float)), None,
                                       WM_SLOT_SYNC))
        return corr[0] if image.dim() == 2 else corr

    def detectOffsets(self, image, keys, k, oy0, ox0, ny, nx, maskType):
        """where does a cropped copy lie in its key?  detectWatermark of `image` against the windows
        keys[k][oy : oy + rows, ox : ox + cols] of a KeySet whose planes are at least as large as the image, at the offsets
        (oy0 + i, ox0 + j), i < ny, j < nx, in one call (wm.h wm_detect_offsets): a float32 numpy array [frames, ny, nx]
        ([ny, nx] for one grey frame); 0.0 at every offset of an unsolvable frame.  The peak is smeared over the 3x3
        neighbourhood of the true offset by the prediction filter: take the argmax"""
        import torch
        pimg = plane_of(image, 1)
        frames = pimg.frames
        corr = np.zeros((frames, max(ny, 0), max(nx, 0)), np.float32)
        torch.cuda.current_stream().synchronize()
        self._chk(lib().wm_detect_offsets(self._ctx, int(maskType), C.byref(pimg), keys.handle, k, oy0, ox0, ny, nx,
                                          corr.ctypes.data_as(_P(C.c_float)), None, WM_SLOT_SYNC))
        return corr[0] if image.dim() == 2 else corr

    def locate(self, image, keys, k, maskType=MASK_TYPE.ME, want_map=False):
        """where does a cropped copy lie in its key, without a hint?  The cross-correlation of the frame's image-side plane with key
        `k` of the KeySet over EVERY admissible offset, by FFT (wm.h wm_locate): a float32 numpy array [frames, 4] ([4] for one grey
        frame) = (oy, ox, peak, z) -- the argmax, the map value there (the detector's <e_u, e_w> against that window) and its
        distance from the rest of the map in standard deviations; zeros for an unsolvable frame.  want_map=True: (loc, map) with map a
        float32 GPU tensor [frames, ny, nx] ([ny, nx])"""
        import torch
        pimg = plane_of(image, 1)
        frames = pimg.frames
        ny, nx, _, _ = locate_shape(self.rows, self.cols, keys.rows, keys.cols)
        loc = np.zeros((frames, WM_LOCATE_NVALS), np.float32)
        map_t = torch.empty((frames, ny, nx), dtype=torch.float32, device=image.device) if want_map else None
        torch.cuda.current_stream().synchronize()
        self.locate_async(image, keys, k, maskType, WM_SLOT_SYNC, loc, map_t)
        one = image.dim() == 2
        if want_map:
            return (loc[0], map_t[0]) if one else (loc, map_t)
        return loc[0] if one else loc

    def locateKeys(self, image, keys, k0, nk, maskType=MASK_TYPE.ME, want_maps=False):
        """whose key is in a cropped copy, and where?  locate() of every frame against keys k0 .. k0 + nk - 1 of the KeySet in one call,
        two keys per transform (wm.h wm_locate_keys): a float32 numpy array [frames, nk, 4] ([nk, 4] for one grey frame) = (oy, ox,
        peak, z) per key; locate_keys_rank names the owner.  Zeros for an unsolvable frame, (0, 0, 0, NaN) for a key plane that is all
        zero.  want_maps=True: (loc, maps) with maps a float32 GPU tensor [frames, nk, ny, nx] ([nk, ny, nx])"""
        import torch
        pimg = plane_of(image, 1)
        frames = pimg.frames
        ny, nx, _, _ = locate_shape(self.rows, self.cols, keys.rows, keys.cols)
        loc = np.zeros((frames, max(nk, 0), WM_LOCATE_KEYS_NVALS), np.float32)
        maps_t = torch.empty((frames, max(nk, 0), ny, nx), dtype=torch.float32, device=image.device) if want_maps else None
        torch.cuda.current_stream().synchronize()
        self.locate_keys_async(image, keys, k0, nk, maskType, WM_SLOT_SYNC, loc, maps_t)
        one = image.dim() == 2
        if want_maps:
            return (loc[0], maps_t[0]) if one else (loc, maps_t)
        return loc[0] if one else loc

    def locate_bits(self, image, keys, k, tile_rows, tile_cols, tile_bit, nbits, maskType=MASK_TYPE.ME, want_energy=False, want_maps=False):
        """finds a cropped, PAYLOAD-marked copy in key `k` of the KeySet and reads its bits (wm.h wm_locate_bits): the tiles (tile_rows x
        tile_cols, tile_bit int32 [ty * tx], -1: no bit) lie on the KEY plane.  Returns (loc, soft[, energy][, maps]): loc a float32
        numpy array [frames, 4] ([4] for one grey frame) = (oy, ox, peak, z) of the energy map sum_b map_b^2, soft float32 [frames,
        nbits] ([nbits]) with bit b = soft > 0 (NaN: a bit without a tile; about 0: no pixel of the bit in the window, see
        locate_bits_cover); energy a float32 GPU tensor [frames, ny, nx], maps [frames, nbits, ny, nx].  Zeros for an unsolvable frame"""
        import torch
        pimg = plane_of(image, 1)
        frames = pimg.frames
        ny, nx, _, _ = locate_shape(self.rows, self.cols, keys.rows, keys.cols)
        loc = np.zeros((frames, WM_LOCATE_BITS_NVALS), np.float32)
        soft = np.zeros((frames, max(nbits, 0)), np.float32)
        en_t = torch.empty((frames, ny, nx), dtype=torch.float32, device=image.device) if want_energy else None
        maps_t = torch.empty((frames, max(nbits, 0), ny, nx), dtype=torch.float32, device=image.device) if want_maps else None
        torch.cuda.current_stream().synchronize()
        self.locate_bits_async(image, keys, k, tile_rows, tile_cols, tile_bit, nbits, maskType, WM_SLOT_SYNC, loc, soft, en_t, maps_t)
        one = image.dim() == 2
        out = [loc[0] if one else loc, soft[0] if one else soft]
        if want_energy:
            out.append(en_t[0] if one else en_t)
        if want_maps:
            out.append(maps_t[0] if one else maps_t)
        return tuple(out)

    # -- a clip's frames pooled into one crop search (wm.h wm_clip_pool, wm_locate_*_pooled) --
    def poolClip(self, frames, maskType=MASK_TYPE.ME, weights=None, pool=None, accumulate=False):
        """the frames of a clip pooled on the image side (wm.h wm_clip_pool): pool = fmaf(w_f, h_f, pool) over the solvable frames in
        ascending order, from zero unless `accumulate`.  frames: [F, rows, cols] (or one [rows, cols] frame), F <= max_frames;
        weights: F floats or None (all 1); pool: a contiguous float32 GPU tensor [rows, cols] or None (a new one).  Returns
        (pool, status) with status an int32 numpy array [F]: an unsolvable frame is skipped and named there"""
        import torch
        pimg = plane_of(frames, 1)
        if pool is None:
            if accumulate:
                raise RuntimeError("poolClip: accumulate needs a pool")
            pool = torch.empty((self.rows, self.cols), dtype=torch.float32, device=frames.device)
        st = np.zeros(pimg.frames, np.int32)
        torch.cuda.current_stream().synchronize()
        self.pool_clip_async(frames, maskType, WM_SLOT_SYNC, pool, weights, accumulate, st)
        return pool, st

    def locatePooled(self, pool, keys, k, want_map=False):
        """locate() of a pooled clip (wm.h wm_locate_pooled): a float32 numpy array [4] = (oy, ox, peak, z); want_map=True: (loc, map)
        with map a float32 GPU tensor [ny, nx]"""
        import torch
        ny, nx, _, _ = locate_shape(self.rows, self.cols, keys.rows, keys.cols)
        loc = np.zeros(WM_LOCATE_NVALS, np.float32)
        map_t = torch.empty((ny, nx), dtype=torch.float32, device=pool.device) if want_map else None
        torch.cuda.current_stream().synchronize()
        self.locate_pooled_async(pool, keys, k, WM_SLOT_SYNC, loc, map_t)
        return (loc, map_t) if want_map else loc

    def locateBitsPooled(self, pool, keys, k, tile_rows, tile_cols, tile_bit, nbits, want_energy=False, want_maps=False):
        """locate_bits() of a pooled clip (wm.h wm_locate_bits_pooled): (loc [4], soft [nbits][, energy [ny, nx]][, maps [nbits, ny, nx]])"""
        import torch
        ny, nx, _, _ = locate_shape(self.rows, self.cols, keys.rows, keys.cols)
        loc = np.zeros(WM_LOCATE_BITS_NVALS, np.float32)
        soft = np.zeros(max(nbits, 0), np.float32)
        en_t = torch.empty((ny, nx), dtype=torch.float32, device=pool.device) if want_energy else None
        maps_t = torch.empty((max(nbits, 0), ny, nx), dtype=torch.float32, device=pool.device) if want_maps else None
        torch.cuda.current_stream().synchronize()
        self.locate_bits_pooled_async(pool, keys, k, tile_rows, tile_cols, tile_bit, nbits, WM_SLOT_SYNC, loc, soft, en_t, maps_t)
        return (loc, soft) + ((en_t,) if want_energy else ()) + ((maps_t,) if want_maps else ())

    def locateKeysPooled(self, pool, keys, k0, nk, want_maps=False):
        """locateKeys() of a pooled clip (wm.h wm_locate_keys_pooled): a float32 numpy array [nk, 4]; want_maps=True: (loc, maps) with
        maps a float32 GPU tensor [nk, ny, nx].  locate_keys_rank names the owner"""
        import torch
        ny, nx, _, _ = locate_shape(self.rows, self.cols, keys.rows, keys.cols)
        loc = np.zeros((max(nk, 0), WM_LOCATE_KEYS_NVALS), np.float32)
        maps_t = torch.empty((max(nk, 0), ny, nx), dtype=torch.float32, device=pool.device) if want_maps else None
        torch.cuda.current_stream().synchronize()
        self.locate_keys_pooled_async(pool, keys, k0, nk, WM_SLOT_SYNC, loc, maps_t)
        return (loc, maps_t) if want_maps else loc

    def locateClip(self, frames, keys, k, maskType=MASK_TYPE.ME, weights=None, want_map=False):
        """where does a cropped CLIP lie in key `k`?  frames [F, rows, cols] of any F: pooled in chunks of max_frames (poolClip), then one locatePooled.  Returns (loc [4], status [F]) or, with
        want_map=True, (loc, status, map)"""
        F, chunk = frames.shape[0], self._max_frames
        w = None if weights is None else np.ascontiguousarray(weights, np.float32).reshape(-1)
        if w is not None and w.size != F:
            raise RuntimeError(f"weights must hold {F} entries, got {w.size}")
        pool, status = None, []
        for f0 in range(0, F, chunk):
            f1 = min(F, f0 + chunk)
            pool, st = self.poolClip(frames[f0:f1], maskType, None if w is None else w[f0:f1], pool, accumulate=f0 > 0)
            status.append(st)
        out = self.locatePooled(pool, keys, k, want_map)
        status = np.concatenate(status)
        return (out[0], status, out[1]) if want_map else (out, status)

    @staticmethod
    def tiles_shape(rows, cols, tile_rows, tile_cols):
        """(ny, nx) of wm_tiles_shape: ny = max(1, rows // tile_rows), nx = max(1, cols // tile_cols); the last tile of each axis
        takes the remainder.  Raises for a tile shape the library refuses (rows: a multiple of 8, >= 32; columns: a multiple of
        4, >= 32)"""
        ny, nx = C.c_int(), C.c_int()
        rc = lib().wm_tiles_shape(rows, cols, tile_rows, tile_cols, C.byref(ny), C.byref(nx))
        if rc != WM_OK:
            _raise(rc)
        return ny.value, nx.value

    def detectTiles(self, image, tile_rows, tile_cols, maskType, sums=False):
        """where in the frame is the mark?  detectWatermark of `image` against the engine's W with the three sums kept per tile
        (wm.h wm_detect_tiles): a float32 numpy array [frames, ny, nx] ([ny, nx] for one grey frame) of tile scores, 0.0 in every
        tile of an unsolvable frame, NaN in a tile without energy.  sums=True: (map, sums) with sums float64 [..., ny, nx, 3] =
        {<e_u,e_w>, |e_u|^2, |e_w|^2} per tile: they add, so any union of tiles is scored from them on the host"""
        import torch
        pimg = plane_of(image, 1)
        frames = pimg.frames
        ny, nx = self.tiles_shape(self.rows, self.cols, tile_rows, tile_cols)
        map_t = torch.empty((frames, ny, nx), dtype=torch.float32, device=image.device)
        sums_t = torch.empty((frames, ny, nx, 3), dtype=torch.float64, device=image.device) if sums else None
        torch.cuda.current_stream().synchronize()
        self.detect_tiles_async(image, tile_rows, tile_cols, maskType, WM_SLOT_SYNC, map_t, sums_t)
        m = map_t.cpu().numpy()
        if image.dim() == 2:
            return (m[0], sums_t.cpu().numpy()[0]) if sums else m[0]
        return (m, sums_t.cpu().numpy()) if sums else m

    def detectKeysTiles(self, image, keys, tile_rows, tile_cols, maskType, sums=False):
        """whose mark is where?  detectTiles of `image` with every key of the KeySet `keys` in the place of the engine's W, in one
        call (wm.h wm_detect_keys_tiles): a float32 numpy array [frames, K, ny, nx] ([K, ny, nx] for one grey frame) of tile
        scores -- the argmax over K names the key a tile was marked with --, 0.0 in every tile of an unsolvable frame, NaN for a
        zero key or a tile without energy.  sums=True: (map, sums) with sums float64 [..., K, ny, nx, 3] =
        {<e_u,e_w>, |e_u|^2, |e_w|^2}: they add over tiles and over the frames of a clip"""
        import torch
        pimg = plane_of(image, 1)
        frames, K = pimg.frames, keys.count
        ny, nx = self.tiles_shape(self.rows, self.cols, tile_rows, tile_cols)
        map_t = torch.empty((frames, K, ny, nx), dtype=torch.float32, device=image.device)
        sums_t = torch.empty((frames, K, ny, nx, 3), dtype=torch.float64, device=image.device) if sums else None
        torch.cuda.current_stream().synchronize()
        self.detect_keys_tiles_async(image, keys, tile_rows, tile_cols, maskType, WM_SLOT_SYNC, map_t, sums_t)
        m = map_t.cpu().numpy()
        if image.dim() == 2:
            return (m[0], sums_t.cpu().numpy()[0]) if sums else m[0]
        return (m, sums_t.cpu().numpy()) if sums else m

    @staticmethod
    def bits_layout(ny, nx, nbits, seed):
        """which bit does tile t carry?  wm_bits_layout's table: an int32 numpy array [ny * nx] with entries 0 .. nbits - 1, every
        bit on floor(T / nbits) or ceil(T / nbits) tiles spread over the frame by a shuffle seeded with `seed`"""
        tb = np.empty(max(ny, 0) * max(nx, 0), np.int32)
        rc = lib().wm_bits_layout(ny, nx, nbits, int(seed) & 0xFFFFFFFFFFFFFFFF, tb.ctypes.data_as(_P(C.c_int32)))
        if rc != WM_OK:
            _raise(rc)
        return tb

    @staticmethod
    def _strength_bufs(frames):
        """(a, st) a synchronous embed delivers into: NaN strengths and zero statuses, one per frame"""
        return (C.c_float * frames)(*([float("nan")] * frames)), (C.c_int * frames)()

    @staticmethod
    def _strengths(a, st, single):
        """the strength, or None for an unsolvable system, of every frame (of the one grey frame: single)"""
        got = [None if st[f] != 0 else a[f] for f in range(len(st))]
        return got[0] if single else got

    def _embed_tiles(self, how, inputImage, outputImage, maskType, out):
        import torch
        if out is None:
            out = torch.empty_like(outputImage)
        a, st = self._strength_bufs(plane_of(inputImage, 1).frames)
        torch.cuda.current_stream().synchronize()
        how(inputImage, outputImage, out, maskType, WM_SLOT_SYNC, a, st)
        return out, self._strengths(a, st, inputImage.dim() == 2)

    def makeWatermarkSigns(self, inputImage, outputImage, tile_rows, tile_cols, signs, maskType, out=None):
        """makeWatermark with the watermark term of every pixel multiplied by the sign of its tile (wm.h wm_embed_signs): `signs`
        is an integer array [ny, nx] ([F, ny, nx] for a batch) of -1, 0 or +1.  Returns (watermarked, strength) as makeWatermark
        does; never takes the fused kernels"""
        return self._embed_tiles(lambda i, b, o, m, slot, a, st: self.embed_signs_async(i, b, o, tile_rows, tile_cols, signs, m, slot, a, st),
                                 inputImage, outputImage, maskType, out)

    def makeWatermarkBits(self, inputImage, outputImage, tile_rows, tile_cols, tile_bit, nbits, payload, maskType, out=None):
        """makeWatermark that carries `payload` (wm.h wm_embed_bits): bytes (or a uint8 array) of (nbits + 7) // 8 bytes per frame,
        bit b = payload[b // 8] >> (b % 8) & 1; tile t is marked with +W where bit tile_bit[t] is set, with -W where it is not, and
        left unmarked where tile_bit[t] = -1 (tile_bit: bits_layout's table or the caller's own).  Returns (watermarked, strength)"""
        return self._embed_tiles(lambda i, b, o, m, slot, a, st: self.embed_bits_async(i, b, o, tile_rows, tile_cols, tile_bit, nbits, payload, m, slot, a, st),
                                 inputImage, outputImage, maskType, out)

    def detectBits(self, image, tile_rows, tile_cols, tile_bit, nbits, maskType):
        """reads the payload back (wm.h wm_detect_bits): (payload, soft) with soft a float32 numpy array [nbits] ([F, nbits] for a
        batch) -- the score of the pooled tiles of every bit, 0.0 for an unsolvable frame, NaN for a bit without a tile -- and
        payload the decoded bits soft > 0 packed as makeWatermarkBits takes them: bytes for one frame, a list of bytes for a batch"""
        import torch
        pimg = plane_of(image, 1)
        frames = pimg.frames
        soft = np.zeros((frames, max(nbits, 0)), np.float32)
        torch.cuda.current_stream().synchronize()
        self.detect_bits_async(image, tile_rows, tile_cols, tile_bit, nbits, maskType, WM_SLOT_SYNC, soft)
        packed = [np.packbits(soft[f] > 0, bitorder="little").tobytes() for f in range(frames)]
        return (packed[0], soft[0]) if image.dim() == 2 else (packed, soft)

    def makeWatermarkKeys(self, inputImage, outputImage, keys, maskType, out=None):
        """makeWatermark of `inputImage` with every key of the KeySet `keys` as W in one call (wm.h wm_embed_keys).  Returns
        (copies, strengths): copies [K, ...] for one frame ([F, K, ...] for a batch [F, R, C]), copy k marked with key k, each
        shaped like one frame of `outputImage`; strengths a float32 numpy array [K] ([F, K]), NaN for every key of an unsolvable
        frame (whose copies equal outputImage).  `out`, if given, is a tensor of the copies' shape on the GPU."""
        import torch
        rgb = outputImage.dim() - inputImage.dim() == 1
        ch = 3 if rgb else 1
        pin = plane_of(inputImage, 1)
        pbase = plane_of(outputImage, ch)
        frames, K = pin.frames, keys.count
        batched = inputImage.dim() == 3
        per = tuple(outputImage.shape[1:] if batched else outputImage.shape)
        shape = ((frames,) if batched else ()) + (K,) + per
        if out is None:
            out = torch.empty(shape, dtype=outputImage.dtype, device=outputImage.device)
        elif tuple(out.shape) != shape or out.dtype != outputImage.dtype:
            raise RuntimeError(f"out must be {outputImage.dtype} of shape {shape}, got {out.dtype} {tuple(out.shape)}")
        pout = plane_of(out.view((frames * K,) + per), ch)
        a = np.full((frames, K), np.nan, np.float32)
        torch.cuda.current_stream().synchronize()
        self._chk(lib().wm_embed_keys(self._ctx, int(maskType), C.byref(pin), C.byref(pbase), keys.handle, C.byref(pout),
                                      a.ctypes.data_as(_P(C.c_float)), None, WM_SLOT_SYNC))
        return out, (a if batched else a[0])

    @staticmethod
    def key_schedule(nkeys, seed, first_frame, frames):
        """which key does frame n of a video take?  wm_key_schedule's table for frames first_frame .. first_frame + frames - 1: an
        int32 numpy array [frames] with entries 0 .. nkeys - 1, entry i a function of (seed, first_frame + i) alone"""
        kt = np.empty(max(frames, 0), np.int32)
        rc = lib().wm_key_schedule(nkeys, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_frame) & 0xFFFFFFFFFFFFFFFF, frames,
                                   kt.ctypes.data_as(_P(C.c_int32)))
        if rc != WM_OK:
            _raise(rc)
        return kt

    def makeWatermarkSelect(self, inputImage, outputImage, keys, key_of_frame, maskType, out=None):
        """makeWatermark of frame f with key key_of_frame[f] of the KeySet `keys` as W (wm.h wm_embed_select): key_of_frame is an
        integer array [F] (one entry, or an int, for one grey frame).  Returns (watermarked, strength) as makeWatermark does; the
        context's own W is not used; never takes the fused kernels"""
        return self._embed_tiles(lambda i, b, o, m, slot, a, st: self.embed_select_async(i, b, o, keys, key_of_frame, m, slot, a, st),
                                 inputImage, outputImage, maskType, out)

    def detectSelect(self, image, keys, key_of_frame, maskType):
        """detectWatermark of frame f against key key_of_frame[f] of the KeySet `keys` (wm.h wm_detect_select): the score of one
        grey frame, a list of scores for a batch; 0.0 for an unsolvable frame"""
        import torch
        frames = plane_of(image, 1).frames
        corr = (C.c_float * frames)()
        torch.cuda.current_stream().synchronize()
        self.detect_select_async(image, keys, key_of_frame, maskType, WM_SLOT_SYNC, corr)
        return corr[0] if image.dim() == 2 else list(corr)

    def _embed_multi(self, how, inputImage, outputImage, K, maskType, out):
        """the synchronous front of the *_multi embeds: K copies per frame shaped as makeWatermarkKeys returns them, one strength per
        frame (NaN for an unsolvable frame, whose copies equal outputImage)"""
        import torch
        batched = inputImage.dim() == 3
        frames = plane_of(inputImage, 1).frames
        per = tuple(outputImage.shape[1:] if batched else outputImage.shape)
        shape = ((frames,) if batched else ()) + (K,) + per
        if out is None:
            out = torch.empty(shape, dtype=outputImage.dtype, device=outputImage.device)
        elif tuple(out.shape) != shape or out.dtype != outputImage.dtype:
            raise RuntimeError(f"out must be {outputImage.dtype} of shape {shape}, got {out.dtype} {tuple(out.shape)}")
        a, st = self._strength_bufs(frames)
        torch.cuda.current_stream().synchronize()
        how(inputImage, outputImage, out.view((frames * K,) + per), maskType, WM_SLOT_SYNC, a, st)
        return out, np.array([np.nan if st[f] != 0 else a[f] for f in range(frames)], np.float32)

    def makeWatermarkSignsMulti(self, inputImage, outputImage, tile_rows, tile_cols, signs, maskType, out=None):
        """one frame, K payload copies in one call (wm.h wm_embed_signs_multi): `signs` is an integer array [F, K, ny, nx] ([K, ny, nx]
        for one frame) of -1, 0 or +1.  Returns (copies, a): copies [F, K, ...] ([K, ...] for one frame) shaped as makeWatermarkKeys
        returns them, copy (f, k) what makeWatermarkSigns writes with signs[f][k]; a float32 [F], one strength per frame"""
        frames = plane_of(inputImage, 1).frames
        K = np.asarray(signs).size // max(1, frames * int(np.prod(self.tiles_shape(self.rows, self.cols, tile_rows, tile_cols))))
        return self._embed_multi(lambda i, b, o, m, slot, a, st: self.embed_signs_multi_async(i, b, o, tile_rows, tile_cols, K, signs, m, slot, a, st),
                                 inputImage, outputImage, K, maskType, out)

    def makeWatermarkBitsMulti(self, inputImage, outputImage, tile_rows, tile_cols, tile_bit, nbits, payloads, maskType, out=None):
        """one frame, K payloads in one call (wm.h wm_embed_bits_multi): `payloads` is a uint8 array [F, K, (nbits + 7) // 8]
        ([K, ...] for one frame) or a list of K bytes objects for one frame.  Returns (copies, a) as makeWatermarkSignsMulti does"""
        frames = plane_of(inputImage, 1).frames
        if isinstance(payloads, (list, tuple)) and payloads and isinstance(payloads[0], (bytes, bytearray)):
            payloads = np.stack([np.frombuffer(bytes(b), np.uint8) for b in payloads])
        K = np.asarray(payloads).size // max(1, frames * ((max(nbits, 1) + 7) // 8))
        return self._embed_multi(lambda i, b, o, m, slot, a, st: self.embed_bits_multi_async(i, b, o, tile_rows, tile_cols, tile_bit, nbits, K, payloads,
                                                                                             m, slot, a, st),
                                 inputImage, outputImage, K, maskType, out)

    def makeAndDetect(self, inputImage, outputImage, maskType, out=None):
        """makeWatermark followed by detectWatermark on its result (testForImage's pair, main.cpp:165-220) as one call
        (wm.h wm_embed_detect; grey output).  Returns (watermarked, strength or None, correlation)."""
        import torch
        pin, pbase = plane_of(inputImage, 1), plane_of(outputImage, 1)
        if out is None:
            out = torch.empty_like(outputImage)
        pout = plane_of(out, 1)
        a, st = self._strength_bufs(pin.frames)
        corr = (C.c_float * pin.frames)()
        torch.cuda.current_stream().synchronize()
        self._chk(lib().wm_embed_detect(self._ctx, int(maskType), C.byref(pin), C.byref(pbase), C.byref(pout), a, corr, st, WM_SLOT_SYNC))
        single = inputImage.dim() == 2
        return out, self._strengths(a, st, single), (corr[0] if single else list(corr))

    # -- pixel formats (wm.h wm_rgb2gray / wm_unpack_rgb8 / wm_pack_rgb8) ------------------------------------------------
    def rgb2gray(self, rgb, weights=None, out=None):
        """af::rgb2gray (main.cpp:153-154): the grey [R, C] ([F, R, C]) float32 of a planar RGB tensor [3, R, C] ([F, 3, R, C]),
        float32 or uint8; weights (r, g, b), default 0.299, 0.587, 0.114; grey = (r R + g G) + b B in f32"""
        import torch
        if out is None:
            out = torch.empty(tuple(rgb.shape[:-3]) + tuple(rgb.shape[-2:]), dtype=torch.float32, device=rgb.device)
        torch.cuda.current_stream().synchronize()
        self.rgb2gray_async(rgb, out, WM_SLOT_SYNC, weights)
        return out

    def unpackRgb8(self, packed, dtype, gray=True):
        """interleaved uint8 pixels [R, C, 3] ([F, R, C, 3]; a GPU tensor, or a CPU tensor that is staged) -> (rgb, grey): the planar
        tensor [3, R, C] ([F, 3, R, C]) of `dtype` (torch.float32 or torch.uint8) and, unless gray is false (then None), its grey
        float32 [R, C] ([F, R, C]) as rgb2gray gives it, both on the engine's device, in one pass over the source"""
        import torch
        dev = packed.device if packed.is_cuda else torch.device("cuda", lib().wm_device(self._ctx))
        lead = tuple(packed.shape[:-3])
        R, Cc = packed.shape[-3], packed.shape[-2]
        rgb = torch.empty(lead + (3, R, Cc), dtype=dtype, device=dev)
        g = torch.empty(lead + (R, Cc), dtype=torch.float32, device=dev) if gray else None
        torch.cuda.current_stream().synchronize()
        self.unpack_rgb8_async(packed, rgb, g, WM_SLOT_SYNC)
        return rgb, g

    def packRgb8(self, rgb, out=None):
        """the .as(u8) in front of saving (main.cpp:235-237): planar [3, R, C] ([F, 3, R, C]) float32 or uint8 -> interleaved uint8
        [R, C, 3] ([F, R, C, 3]); float32 is clamped to [0, 255] and truncated, NaN gives 0.  `out`: a uint8 tensor of that shape
        on the GPU, or on the CPU (then the pixels are downloaded into it)"""
        import torch
        if out is None:
            out = torch.empty(tuple(rgb.shape[:-3]) + tuple(rgb.shape[-2:]) + (3,), dtype=torch.uint8, device=rgb.device)
        torch.cuda.current_stream().synchronize()
        self.pack_rgb8_async(rgb, out, WM_SLOT_SYNC)
        return out

    # -- samples of 9 to 16 bits (wm.h wm_unpack16 / wm_pack16 / wm_embed16 / wm_detect16) ---------------------------------
    # samples: numpy uint16 arrays or torch uint16 / int16 tensors (CPU: staged; GPU: device planes), [R,C] or [F,R,C]
    def _dev(self):
        import torch
        return torch.device("cuda", lib().wm_device(self._ctx))

    def unpack16(self, samples, bits, msbAligned=False, channels=1, out=None):
        """`bits`-bit samples -> float32 on [0, 255] on the engine's device: min(v, 2^bits - 1) * k_in (msbAligned: v >> (16 - bits))"""
        import torch
        if out is None:
            out = torch.empty(tuple(samples.shape), dtype=torch.float32, device=self._dev())
        torch.cuda.current_stream().synchronize()
        self.unpack16_async(samples, bits, out, WM_SLOT_SYNC, msbAligned, channels)
        return out

    def pack16(self, image, bits, msbAligned=False, channels=1, out=None):
        """float32 on [0, 255] -> `bits`-bit samples, clamped and rounded to nearest (ties to even), NaN gives 0.  `out`: a 16-bit
        array or tensor of image's shape; default a new numpy uint16 array (the samples are downloaded)"""
        import numpy as np
        import torch
        if out is None:
            out = np.empty(tuple(image.shape), dtype=np.uint16)
        torch.cuda.current_stream().synchronize()
        self.pack16_async(image, out, bits, WM_SLOT_SYNC, msbAligned, channels)
        return out

    def makeWatermark16(self, samples, bits, maskType, msbAligned=False, out=None):
        """makeWatermark of grey `bits`-bit frames (wm.h wm_embed16): unpack, embed onto the frame itself, pack.  `out`: where the
        marked samples go, `samples` itself for an in-place call; default a new array like `samples`.  Returns (out, strength)"""
        import numpy as np
        import torch
        if out is None:
            out = np.empty_like(samples) if isinstance(samples, np.ndarray) else torch.empty_like(samples)
        pin = plane_any(samples, 1)
        a, st = self._strength_bufs(pin.frames)
        torch.cuda.current_stream().synchronize()
        self.embed16_async(pin, out, bits, maskType, WM_SLOT_SYNC, msbAligned, a, st)
        return out, self._strengths(a, st, len(samples.shape) == 2)

    def detectWatermark16(self, samples, bits, maskType, msbAligned=False):
        """detectWatermark of grey `bits`-bit frames (wm.h wm_detect16); 0.0 for an unsolvable system"""
        import torch
        pimg = plane_any(samples, 1)
        corr = (C.c_float * pimg.frames)()
        torch.cuda.current_stream().synchronize()
        self.detect16_async(pimg, bits, maskType, WM_SLOT_SYNC, msbAligned, corr)
        return corr[0] if len(samples.shape) == 2 else list(corr)

    # -- quality of a marked copy (wm.h wm_quality) ---------------------------------------------------------------------------
    def quality(self, ref, test, tile=None, sums=False, channels=1):
        """PSNR and SSIM of `test` against `ref`, measured on the device (wm.h wm_quality): (mse, psnr, ssim, maxabs), float64 numpy
        arrays [frames, channels]; psnr = psnr_from_mse(mse, 255), ssim is NaN for planes below 11 x 11.  ref / test: float32 or uint8
        arrays -- GPU tensors, CPU tensors or numpy arrays (staged), or wm_planes (test may be a WM_MEM_SLOT_OUT plane) --, [R,C],
        [3,R,C] with channels=3, or a batch of either.  tile=(tile_rows, tile_cols) chooses the tile grid of the sums (default: one
        tile per plane); sums=True appends them: float64 [frames, channels, ny, nx, 5] = {sse, npix, ssim_sum, nwin, max|d|}"""
        import torch
        pr, pt = self._as_plane_u8f32(ref, channels), self._as_plane_u8f32(test, channels)
        F, ch = pr.frames, pr.channels
        tile_rows, tile_cols = tile if tile is not None else (0, 0)
        ny, nx = self.tiles_shape(self.rows, self.cols, tile_rows, tile_cols) if tile is not None else (1, 1)
        q = np.zeros((F, ch, WM_QUALITY_NVALS), np.float32)
        sums_t = torch.empty((F, ch, ny, nx, WM_QUALITY_NSUMS), dtype=torch.float64, device=self._dev()) if sums else None
        torch.cuda.current_stream().synchronize()
        self.quality_async(pr, pt, WM_SLOT_SYNC, q, tile_rows, tile_cols, sums_t)
        mse = q[..., 0].astype(np.float64)
        psnr = np.array([[psnr_from_mse(v, 255.0) for v in row] for row in mse], np.float64).reshape(F, ch)
        out = (mse, psnr, q[..., 1].astype(np.float64), q[..., 2].astype(np.float64))
        return out + (sums_t.cpu().numpy(),) if sums else out

    @staticmethod
    def _as_plane_u8f32(t, channels):
        return t if isinstance(t, wm_plane) else plane_u8f32(t, channels)

    def quality_async(self, ref, test, slot, q_out, tile_rows=0, tile_cols=0, sums_t=None, channels=1):
        """wm_quality enqueued on `slot`: q_out (frames * channels * 3 floats: a ctypes array or a C-contiguous float32 numpy array,
        may be None) is written by sync(slot); sums_t (a contiguous float64 GPU tensor of frames * channels * ny * nx * 5 elements,
        may be None) on the slot's stream, valid after sync(slot).  Host planes must stay alive until then"""
        pr, pt = self._as_plane_u8f32(ref, channels), self._as_plane_u8f32(test, channels)
        psums = None
        if sums_t is not None:
            import torch
            ny, nx = self.tiles_shape(self.rows, self.cols, tile_rows, tile_cols) if (tile_rows or tile_cols) else (1, 1)
            n = pr.frames * pr.channels * ny * nx * WM_QUALITY_NSUMS
            if not (sums_t.is_cuda and sums_t.dtype == torch.float64 and sums_t.is_contiguous() and sums_t.numel() == n):
                raise RuntimeError(f"sums_t must be a contiguous float64 GPU tensor of {n} elements")
            psums = C.c_void_p(sums_t.data_ptr())
        q_out, _ = self._scalars_out(q_out, None)
        self._chk(lib().wm_quality(self._ctx, C.byref(pr), C.byref(pt), tile_rows, tile_cols, q_out, psums, slot))

    # north_star aliases
    embed = makeWatermark
    detect = detectWatermark

    # -- asynchronous slot interface (frames in flight; wm.h) --------------------------------------
    # `inputImage` / `outputImage` / `out` / `image` may be torch tensors or wm_plane structs prepared once with
    # plane_of(): a streaming loop that reuses its frame buffers should pass planes (no per-call tensor walk)
    @staticmethod
    def _as_plane(t, channels):
        return t if isinstance(t, wm_plane) else plane_of(t, channels)

    def embed_async(self, inputImage, outputImage, out, maskType, slot, a_out=None, status_out=None):
        pin, pbase, pout = self._embed_planes(inputImage, outputImage, out)
        self._chk(lib().wm_embed(self._ctx, int(maskType), C.byref(pin), C.byref(pbase), C.byref(pout), a_out, status_out, slot))

    def detect_async(self, image, maskType, slot, corr_out=None, status_out=None):
        pimg = self._as_plane(image, 1)
        self._chk(lib().wm_detect(self._ctx, int(maskType), C.byref(pimg), corr_out, status_out, slot))

    def detect_keys_async(self, image, keys, maskType, slot, corr_out, status_out=None):
        """wm_detect_keys enqueued on `slot`: corr_out (frames * K floats: a ctypes array or a C-contiguous float32 numpy array)
        and status_out (frames ints, may be None) are written by sync(slot); `keys` must stay alive and unmodified until then"""
        pimg = self._as_plane(image, 1)
        corr_out, status_out = self._scalars_out(corr_out, status_out)
        self._chk(lib().wm_detect_keys(self._ctx, int(maskType), C.byref(pimg), _keys_handle(keys),
                                       corr_out, status_out, slot))

    def detect_offsets_async(self, image, keys, k, oy0, ox0, ny, nx, maskType, slot, corr_out, status_out=None):
        """wm_detect_offsets enqueued on `slot`: corr_out (frames * ny * nx floats: a ctypes array or a C-contiguous float32 numpy
        array) and status_out (frames ints, may be None) are written by sync(slot); `keys` must stay alive and unmodified until
        then"""
        pimg = self._as_plane(image, 1)
        corr_out, status_out = self._scalars_out(corr_out, status_out)
        self._chk(lib().wm_detect_offsets(self._ctx, int(maskType), C.byref(pimg), _keys_handle(keys),
                                          k, oy0, ox0, ny, nx, corr_out, status_out, slot))

    def locate_async(self, image, keys, k, maskType, slot, loc_out, map_t=None, status_out=None):
        """wm_locate enqueued on `slot`: loc_out (frames * 4 floats: a ctypes array or a C-contiguous float32 numpy array, may be None
        when map_t is given) and status_out (frames ints, may be None) are written by sync(slot); map_t (a contiguous float32 GPU
        tensor of frames * ny * nx elements, may be None) is written on the slot's stream.  `keys` must stay alive and unmodified until
        then"""
        pimg = self._as_plane(image, 1)
        loc_out, status_out = self._scalars_out(loc_out, status_out)
        self._chk(lib().wm_locate(self._ctx, int(maskType), C.byref(pimg), _keys_handle(keys), k, loc_out, self._f32_gpu(map_t, "map_t"), status_out,
                                  slot))

    def locate_keys_async(self, image, keys, k0, nk, maskType, slot, loc_out, maps_t=None, status_out=None):
        """wm_locate_keys enqueued on `slot`: loc_out (frames * nk * 4 floats: a ctypes array or a C-contiguous float32 numpy array, may
        be None when maps_t is given) and status_out (frames ints, may be None) are written by sync(slot); maps_t (a contiguous float32
        GPU tensor of frames * nk * ny * nx elements, may be None) is written on the slot's stream.  `keys` must stay alive and
        unmodified until then"""
        pimg = self._as_plane(image, 1)
        loc_out, status_out = self._scalars_out(loc_out, status_out)
        self._chk(lib().wm_locate_keys(self._ctx, int(maskType), C.byref(pimg), _keys_handle(keys), k0, nk, loc_out, self._f32_gpu(maps_t, "maps_t"),
                                       status_out, slot))

    def locate_bits_async(self, image, keys, k, tile_rows, tile_cols, tile_bit, nbits, maskType, slot, loc_out, soft_out, energy_t=None,
                          maps_t=None, status_out=None):
        """wm_locate_bits enqueued on `slot`: tile_bit (int32, one entry per tile of the KEY plane) is read before the call returns;
        loc_out (frames * 4 floats), soft_out (frames * nbits floats) and status_out (frames ints, may be None) are written by
        sync(slot); energy_t (frames * ny * nx) and maps_t (frames * nbits * ny * nx), contiguous float32 GPU tensors that may be
        None, on the slot's stream.  `keys` must stay alive and unmodified until then"""
        pimg = self._as_plane(image, 1)
        tb = self._key_tile_table(keys, tile_rows, tile_cols, tile_bit)
        loc_out, status_out = self._scalars_out(loc_out, status_out)
        soft_out, _ = self._scalars_out(soft_out, None)
        self._chk(lib().wm_locate_bits(self._ctx, int(maskType), C.byref(pimg), _keys_handle(keys), k, tile_rows, tile_cols,
                                       tb.ctypes.data_as(C.c_void_p) if tb is not None else None, nbits, loc_out, soft_out,
                                       self._f32_gpu(energy_t, "energy_t"), self._f32_gpu(maps_t, "maps_t"), status_out, slot))

    @staticmethod
    def _key_tile_table(keys, tile_rows, tile_cols, tile_bit):
        """tile_bit as a flat int32 array with one entry per tile of the KEY plane (a tile shape the library refuses, and None, pass
        through to its own refusal)"""
        tb = np.ascontiguousarray(tile_bit, np.int32).reshape(-1) if tile_bit is not None else None
        if tb is not None and keys is not None:
            tny, tnx = C.c_int(), C.c_int()
            if lib().wm_tiles_shape(keys.rows, keys.cols, tile_rows, tile_cols, C.byref(tny), C.byref(tnx)) == WM_OK and tb.size != tny.value * tnx.value:
                raise RuntimeError(f"tile_bit must hold {tny.value * tnx.value} entries, got {tb.size}")
        return tb

    @staticmethod
    def _f32_gpu(t, what, n=None):
        """a contiguous float32 GPU tensor (of n elements) as a pointer; None passes through"""
        import torch
        if t is None:
            return None
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and (n is None or t.numel() == n)):
            raise RuntimeError(f"{what} must be a contiguous float32 GPU tensor" + (f" of {n} elements" if n is not None else ""))
        return C.c_void_p(t.data_ptr())

    def pool_clip_async(self, frames, maskType, slot, pool_t, weights=None, accumulate=False, status_out=None):
        """wm_clip_pool enqueued on `slot`: pool_t (a contiguous float32 GPU tensor of rows * cols elements) is written on the slot's
        stream; weights (frames floats, may be None) is read before the call returns; status_out (frames ints, may be None) is
        written by sync(slot)"""
        pimg = self._as_plane(frames, 1)
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, np.float32).reshape(-1)
            if w.size != pimg.frames:
                raise RuntimeError(f"weights must hold {pimg.frames} entries, got {w.size}")
        _, status_out = self._scalars_out(None, status_out)
        self._chk(lib().wm_clip_pool(self._ctx, int(maskType), C.byref(pimg), w.ctypes.data_as(_P(C.c_float)) if w is not None else None,
                                     self._f32_gpu(pool_t, "pool_t", self.rows * self.cols), 1 if accumulate else 0, status_out, slot))

    def locate_pooled_async(self, pool_t, keys, k, slot, loc_out, map_t=None):
        """wm_locate_pooled enqueued on `slot`: loc_out (4 floats, may be None when map_t is given) is written by sync(slot), map_t
        (ny * nx, may be None) on the slot's stream.  `keys` and pool_t must stay alive and unmodified until then"""
        loc_out, _ = self._scalars_out(loc_out, None)
        self._chk(lib().wm_locate_pooled(self._ctx, self._f32_gpu(pool_t, "pool_t", self.rows * self.cols), _keys_handle(keys), k, loc_out,
                                         self._f32_gpu(map_t, "map_t"), slot))

    def locate_bits_pooled_async(self, pool_t, keys, k, tile_rows, tile_cols, tile_bit, nbits, slot, loc_out, soft_out, energy_t=None, maps_t=None):
        """wm_locate_bits_pooled enqueued on `slot`: tile_bit is read before the call returns; loc_out (4 floats) and soft_out (nbits
        floats) are written by sync(slot), energy_t (ny * nx) and maps_t (nbits * ny * nx), which may be None, on the slot's stream"""
        tb = self._key_tile_table(keys, tile_rows, tile_cols, tile_bit)
        loc_out, _ = self._scalars_out(loc_out, None)
        soft_out, _ = self._scalars_out(soft_out, None)
        self._chk(lib().wm_locate_bits_pooled(self._ctx, self._f32_gpu(pool_t, "pool_t", self.rows * self.cols), _keys_handle(keys), k, tile_rows,
                                              tile_cols, tb.ctypes.data_as(C.c_void_p) if tb is not None else None, nbits, loc_out, soft_out,
                                              self._f32_gpu(energy_t, "energy_t"), self._f32_gpu(maps_t, "maps_t"), slot))

    def locate_keys_pooled_async(self, pool_t, keys, k0, nk, slot, loc_out, maps_t=None):
        """wm_locate_keys_pooled enqueued on `slot`: loc_out (nk * 4 floats, may be None when maps_t is given) is written by
        sync(slot), maps_t (nk * ny * nx, may be None) on the slot's stream"""
        loc_out, _ = self._scalars_out(loc_out, None)
        self._chk(lib().wm_locate_keys_pooled(self._ctx, self._f32_gpu(pool_t, "pool_t", self.rows * self.cols), _keys_handle(keys), k0, nk, loc_out,
                                              self._f32_gpu(maps_t, "maps_t"), slot))

    def detect_tiles_async(self, image, tile_rows, tile_cols, maskType, slot, map_t, sums_t=None, status=None):
        """wm_detect_tiles enqueued on `slot`: map_t (a contiguous float32 GPU tensor of frames * ny * nx elements) and sums_t
        (float64, frames * ny * nx * 3, may be None) are written on the slot's stream and valid after sync(slot); status (frames
        ints: a ctypes array or a C-contiguous int32 numpy array, may be None) is written by sync(slot)"""
        pimg = self._as_plane(image, 1)
        ny, nx = self.tiles_shape(self.rows, self.cols, tile_rows, tile_cols)
        n = pimg.frames * ny * nx
        pmap, psums = self._tile_tensors(map_t, sums_t, n)
        _, status = self._scalars_out(None, status)
        self._chk(lib().wm_detect_tiles(self._ctx, int(maskType), C.byref(pimg), tile_rows, tile_cols, pmap, psums, status, slot))

    def detect_keys_tiles_async(self, image, keys, tile_rows, tile_cols, maskType, slot, map_t, sums_t=None, status=None):
        """wm_detect_keys_tiles enqueued on `slot`: map_t (a contiguous float32 GPU tensor of frames * K * ny * nx elements) and
        sums_t (float64, three times as many, may be None) are written on the slot's stream and valid after sync(slot); status
        (frames ints: a ctypes array or a C-contiguous int32 numpy array, may be None) is written by sync(slot); `keys` must stay
        alive and unmodified until then"""
        pimg = self._as_plane(image, 1)
        ny, nx = self.tiles_shape(self.rows, self.cols, tile_rows, tile_cols)
        K = keys.count if isinstance(keys, KeySet) else lib().wm_keys_count(keys)
        n = pimg.frames * K * ny * nx
        pmap, psums = self._tile_tensors(map_t, sums_t, n)
        _, status = self._scalars_out(None, status)
        self._chk(lib().wm_detect_keys_tiles(self._ctx, int(maskType), C.byref(pimg), _keys_handle(keys),
                                             tile_rows, tile_cols, pmap, psums, status, slot))

    def embed_keys_async(self, inputImage, outputImage, out, keys, maskType, slot, a_out=None, status_out=None):
        """wm_embed_keys enqueued on `slot`: `out` holds frames * K copies (a tensor [frames * K, ...] or a wm_plane; copy (f, k) is
        frame f * K + k); a_out (frames * K floats) and status_out (frames ints) -- ctypes arrays or C-contiguous numpy arrays, may
        be None -- are written by sync(slot); `keys` must stay alive and unmodified until then.  With a wm_plane inputImage,
        outputImage is a wm_plane as well (its channels cannot be told from a tensor's rank then)"""
        pin, pbase, pout = self._embed_planes(inputImage, outputImage, out)
        a_out, status_out = self._scalars_out(a_out, status_out)
        self._chk(lib().wm_embed_keys(self._ctx, int(maskType), C.byref(pin), C.byref(pbase), _keys_handle(keys),
                                      C.byref(pout), a_out, status_out, slot))

    def _key_table(self, key_of_frame, frames):
        """the table of a select call as a pointer (None: a null pointer, which the library refuses)"""
        if key_of_frame is None:
            return None, None
        raw = np.atleast_1d(np.asarray(key_of_frame))
        if raw.size and (raw.min() < -2 ** 31 or raw.max() > 2 ** 31 - 1):  # (values the int32 table cannot hold)
            _raise(WM_ERR_BAD_ARG)
        kt = self._host_table(raw, np.int32, frames, "key_of_frame")
        return kt, kt.ctypes.data_as(_P(C.c_int32))

    def embed_select_async(self, inputImage, outputImage, out, keys, key_of_frame, maskType, slot, a_out=None, status_out=None):
        """wm_embed_select enqueued on `slot`: key_of_frame (frames integers in 0 .. K - 1) is copied before the call returns; a_out
        (frames floats) and status_out (frames ints) -- ctypes arrays or C-contiguous numpy arrays, may be None -- are written by
        sync(slot); `keys` must stay alive and unmodified until then"""
        pin, pbase, pout = self._embed_planes(inputImage, outputImage, out)
        kt, pk = self._key_table(key_of_frame, pin.frames)
        a_out, status_out = self._scalars_out(a_out, status_out)
        self._chk(lib().wm_embed_select(self._ctx, int(maskType), C.byref(pin), C.byref(pbase), C.byref(pout), _keys_handle(keys), pk,
                                        a_out, status_out, slot))

    def detect_select_async(self, image, keys, key_of_frame, maskType, slot, corr_out, status_out=None):
        """wm_detect_select enqueued on `slot`: key_of_frame (frames integers in 0 .. K - 1) is copied before the call returns;
        corr_out (frames floats) and status_out (frames ints, may be None) are written by sync(slot); `keys` must stay alive and
        unmodified until then"""
        pimg = self._as_plane(image, 1)
        kt, pk = self._key_table(key_of_frame, pimg.frames)
        corr_out, status_out = self._scalars_out(corr_out, status_out)
        self._chk(lib().wm_detect_select(self._ctx, int(maskType), C.byref(pimg), _keys_handle(keys), pk, corr_out, status_out, slot))

    @staticmethod
    def _host_table(a, dtype, n, what):
        t = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
        if t.size != n:
            raise RuntimeError(f"{what} must hold {n} entries, got {t.size}")
        return t

    @staticmethod
    def _scalars_out(a_out, status_out):
        if isinstance(a_out, np.ndarray):
            assert a_out.dtype == np.float32 and a_out.flags.c_contiguous
            a_out = a_out.ctypes.data_as(_P(C.c_float))
        if isinstance(status_out, np.ndarray):
            assert status_out.dtype == np.int32 and status_out.flags.c_contiguous
            status_out = status_out.ctypes.data_as(_P(C.c_int))
        return a_out, status_out

    @staticmethod
    def _tile_tensors(map_t, sums_t, n):
        """the device tensors of the tiles calls as pointers: map_t n float32, sums_t (may be None) 3 n float64, both contiguous"""
        import torch
        if not (map_t.is_cuda and map_t.dtype == torch.float32 and map_t.is_contiguous() and map_t.numel() == n):
            raise RuntimeError(f"map_t must be a contiguous float32 GPU tensor of {n} elements")
        if sums_t is not None and not (sums_t.is_cuda and sums_t.dtype == torch.float64 and sums_t.is_contiguous() and sums_t.numel() == 3 * n):
            raise RuntimeError(f"sums_t must be a contiguous float64 GPU tensor of {3 * n} elements")
        return C.c_void_p(map_t.data_ptr()), (C.c_void_p(sums_t.data_ptr()) if sums_t is not None else None)

    def _embed_planes(self, inputImage, outputImage, out):
        if isinstance(outputImage, wm_plane):
            ch = outputImage.channels
        elif isinstance(inputImage, wm_plane):
            raise RuntimeError("with a wm_plane inputImage, pass outputImage as a wm_plane too")
        else:
            ch = 3 if outputImage.dim() - inputImage.dim() == 1 else 1
        return self._as_plane(inputImage, 1), self._as_plane(outputImage, ch), self._as_plane(out, ch)

    def embed_signs_async(self, inputImage, outputImage, out, tile_rows, tile_cols, signs, maskType, slot, a_out=None, status_out=None):
        """wm_embed_signs enqueued on `slot`: `signs` (frames * ny * nx integers of -1, 0, +1) is copied before the call returns;
        a_out (frames floats) and status_out (frames ints) -- ctypes arrays or C-contiguous numpy arrays, may be None -- are
        written by sync(slot)"""
        pin, pbase, pout = self._embed_planes(inputImage, outputImage, out)
        ny, nx = self.tiles_shape(self.rows, self.cols, tile_rows, tile_cols)
        raw = np.asarray(signs)
        if raw.dtype != np.int8 and raw.size and (raw.min() < -128 or raw.max() > 127):  # (values the int8 table cannot hold)
            _raise(WM_ERR_BAD_ARG)
        sg = self._host_table(raw, np.int8, pin.frames * ny * nx, "signs")
        a_out, status_out = self._scalars_out(a_out, status_out)
        self._chk(lib().wm_embed_signs(self._ctx, int(maskType), C.byref(pin), C.byref(pbase), C.byref(pout), tile_rows, tile_cols,
                                       sg.ctypes.data_as(C.c_void_p), a_out, status_out, slot))

    def embed_bits_async(self, inputImage, outputImage, out, tile_rows, tile_cols, tile_bit, nbits, payload, maskType, slot, a_out=None,
                         status_out=None):
        """wm_embed_bits enqueued on `slot`: tile_bit (ny * nx int32) and payload (frames * ((nbits + 7) // 8) bytes: bytes or a uint8
        array) are read before the call returns; a_out / status_out as for embed_signs_async"""
        pin, pbase, pout = self._embed_planes(inputImage, outputImage, out)
        ny, nx = self.tiles_shape(self.rows, self.cols, tile_rows, tile_cols)
        tb = self._host_table(tile_bit, np.int32, ny * nx, "tile_bit")
        if isinstance(payload, (bytes, bytearray)):
            payload = np.frombuffer(bytes(payload), np.uint8)
        pl = self._host_table(payload, np.uint8, pin.frames * ((max(nbits, 1) + 7) // 8), "payload")
        a_out, status_out = self._scalars_out(a_out, status_out)
        self._chk(lib().wm_embed_bits(self._ctx, int(maskType), C.byref(pin), C.byref(pbase), C.byref(pout), tile_rows, tile_cols,
                                      tb.ctypes.data_as(C.c_void_p), nbits, pl.ctypes.data_as(C.c_void_p), a_out, status_out, slot))

    def embed_signs_multi_async(self, inputImage, outputImage, out, tile_rows, tile_cols, ncopies, signs, maskType, slot, a_out=None,
                                status_out=None):
        """wm_embed_signs_multi enqueued on `slot`: `out` holds frames * ncopies copies (a tensor [frames * ncopies, ...] or a wm_plane;
        copy (f, k) is frame f * ncopies + k); `signs` (frames * ncopies * ny * nx integers of -1, 0, +1) is copied before the call
        returns; a_out (frames floats) and status_out (frames ints) as for embed_signs_async"""
        pin, pbase, pout = self._embed_planes(inputImage, outputImage, out)
        ny, nx = self.tiles_shape(self.rows, self.cols, tile_rows, tile_cols)
        raw = np.asarray(signs)
        if raw.dtype != np.int8 and raw.size and (raw.min() < -128 or raw.max() > 127):  # (values the int8 table cannot hold)
            _raise(WM_ERR_BAD_ARG)
        sg = self._host_table(raw, np.int8, pin.frames * max(ncopies, 0) * ny * nx, "signs")
        a_out, status_out = self._scalars_out(a_out, status_out)
        self._chk(lib().wm_embed_signs_multi(self._ctx, int(maskType), C.byref(pin), C.byref(pbase), C.byref(pout), tile_rows, tile_cols, ncopies,
                                             sg.ctypes.data_as(C.c_void_p), a_out, status_out, slot))

    def embed_bits_multi_async(self, inputImage, outputImage, out, tile_rows, tile_cols, tile_bit, nbits, ncopies, payloads, maskType, slot,
                               a_out=None, status_out=None):
        """wm_embed_bits_multi enqueued on `slot`: tile_bit (ny * nx int32) and payloads (frames * ncopies * ((nbits + 7) // 8) bytes)
        are read before the call returns; `out`, a_out and status_out as for embed_signs_multi_async"""
        pin, pbase, pout = self._embed_planes(inputImage, outputImage, out)
        ny, nx = self.tiles_shape(self.rows, self.cols, tile_rows, tile_cols)
        tb = self._host_table(tile_bit, np.int32, ny * nx, "tile_bit")
        pl = self._host_table(payloads, np.uint8, pin.frames * max(ncopies, 0) * ((max(nbits, 1) + 7) // 8), "payloads")
        a_out, status_out = self._scalars_out(a_out, status_out)
        self._chk(lib().wm_embed_bits_multi(self._ctx, int(maskType), C.byref(pin), C.byref(pbase), C.byref(pout), tile_rows, tile_cols,
                                            tb.ctypes.data_as(C.c_void_p), nbits, ncopies, pl.ctypes.data_as(C.c_void_p), a_out, status_out, slot))

    def detect_bits_async(self, image, tile_rows, tile_cols, tile_bit, nbits, maskType, slot, soft_out, status_out=None):
        """wm_detect_bits enqueued on `slot`: tile_bit (ny * nx int32) is read before the call returns; soft_out (frames * nbits
        floats: a ctypes array or a C-contiguous float32 numpy array) and status_out (frames ints, may be None) are written by
        sync(slot)"""
        pimg = self._as_plane(image, 1)
        ny, nx = self.tiles_shape(self.rows, self.cols, tile_rows, tile_cols)
        tb = self._host_table(tile_bit, np.int32, ny * nx, "tile_bit")
        soft_out, status_out = self._scalars_out(soft_out, status_out)
        self._chk(lib().wm_detect_bits(self._ctx, int(maskType), C.byref(pimg), tile_rows, tile_cols, tb.ctypes.data_as(C.c_void_p), nbits,
                                       soft_out, status_out, slot))

    @staticmethod
    def _as_packed(t):
        return t if isinstance(t, wm_packed) else packed_of(t)

    @staticmethod
    def _weights(weights):
        return None if weights is None else (C.c_float * 3)(*[float(v) for v in weights])

    def rgb2gray_async(self, rgb, gray_out, slot, weights=None):
        """wm_rgb2gray enqueued on `slot`: rgb a planar tensor [3, R, C] / [F, 3, R, C] or a 3-channel wm_plane (WM_MEM_SLOT_OUT: the
        slot's last 3-channel embed output), gray_out a float32 tensor [R, C] / [F, R, C] or a wm_plane; weights (r, g, b) or None"""
        prgb, pg = self._as_plane(rgb, 3), self._as_plane(gray_out, 1)
        self._chk(lib().wm_rgb2gray(self._ctx, C.byref(prgb), C.byref(pg), self._weights(weights), slot))

    def unpack_rgb8_async(self, packed, rgb_out, gray_out, slot, weights=None):
        """wm_unpack_rgb8 enqueued on `slot`: packed a uint8 tensor [R, C, 3] / [F, R, C, 3] (packed_of) or a wm_packed; rgb_out
        (planar, float32 or uint8) and gray_out (float32) tensors or wm_planes, either may be None"""
        pp = self._as_packed(packed)
        pr = None if rgb_out is None else self._as_plane(rgb_out, 3)
        pg = None if gray_out is None else self._as_plane(gray_out, 1)
        self._chk(lib().wm_unpack_rgb8(self._ctx, C.byref(pp), C.byref(pr) if pr is not None else None, C.byref(pg) if pg is not None else None,
                                       self._weights(weights), slot))

    def pack_rgb8_async(self, rgb, packed_out, slot):
        """wm_pack_rgb8 enqueued on `slot`: rgb as for rgb2gray_async, packed_out a uint8 tensor [R, C, 3] / [F, R, C, 3] or a
        wm_packed"""
        prgb, pp = self._as_plane(rgb, 3), self._as_packed(packed_out)
        self._chk(lib().wm_pack_rgb8(self._ctx, C.byref(prgb), C.byref(pp), slot))

    @staticmethod
    def _as_plane_any(t, channels):
        return t if isinstance(t, wm_plane) else plane_any(t, channels)

    def unpack16_async(self, samples, bits, out_f32, slot, msbAligned=False, channels=1):
        """wm_unpack16 enqueued on `slot`: samples / out_f32 arrays or tensors (plane_any) or wm_planes"""
        ps, po = self._as_plane_any(samples, channels), self._as_plane_any(out_f32, channels)
        self._chk(lib().wm_unpack16(self._ctx, C.byref(ps), int(bits), int(msbAligned), C.byref(po), slot))

    def pack16_async(self, src_f32, out16, bits, slot, msbAligned=False, channels=1):
        """wm_pack16 enqueued on `slot`: src_f32 may be a WM_MEM_SLOT_OUT wm_plane (the slot's last f32 embed output)"""
        ps, po = self._as_plane_any(src_f32, channels), self._as_plane_any(out16, channels)
        self._chk(lib().wm_pack16(self._ctx, C.byref(ps), C.byref(po), int(bits), int(msbAligned), slot))

    def embed16_async(self, in16, out16, bits, maskType, slot, msbAligned=False, a_out=None, status_out=None):
        """wm_embed16 enqueued on `slot`: grey frames, out16 may be in16"""
        pi, po = self._as_plane_any(in16, 1), self._as_plane_any(out16, 1)
        self._chk(lib().wm_embed16(self._ctx, int(maskType), C.byref(pi), C.byref(po), int(bits), int(msbAligned), a_out, status_out, slot))

    def detect16_async(self, img16, bits, maskType, slot, msbAligned=False, corr_out=None, status_out=None):
        """wm_detect16 enqueued on `slot`"""
        pi = self._as_plane_any(img16, 1)
        self._chk(lib().wm_detect16(self._ctx, int(maskType), C.byref(pi), int(bits), int(msbAligned), corr_out, status_out, slot))

    def sync(self, slot):
        return self._chk(lib().wm_sync(self._ctx, slot))

    # -- parity-test building blocks (private in the reference: Watermark.cpp:96-114,176-218) -------------
    def computeMask(self, inputImage, maskType, want_error_sequence=False):
        """returns (mask, e or None, coefficients[8] or None, status)"""
        import torch
        pin = plane_of(inputImage, 1)
        m = torch.empty(inputImage.shape, dtype=torch.float32, device=inputImage.device)
        e = torch.empty_like(m) if want_error_sequence else None
        pm = plane_of(m, 1)
        pe = plane_of(e, 1) if e is not None else None
        frames = pin.frames
        coef = (C.c_float * (8 * frames))()
        st = (C.c_int * frames)()
        torch.cuda.current_stream().synchronize()
        self._chk(lib().wm_compute_mask(self._ctx, int(maskType), C.byref(pin), C.byref(pm), C.byref(pe) if pe else None, coef,
                                        st, WM_SLOT_SYNC))
        c = np.array(coef[:], dtype=np.float32).reshape(frames, 8)
        if inputImage.dim() == 2:
            return m, e, c[0], st[0]
        return m, e, c, list(st)

    def gram(self, image):
        """(Rx [8,8] f64, rx [8] f64) of a grey image: the sums the me kernel + af::sum produce"""
        tot = self.gram_totals(image)[:44]
        Rx = np.zeros((8, 8))
        k = 0
        for i in range(8):
            for j in range(i, 8):
                Rx[i, j] = Rx[j, i] = tot[k]
                k += 1
        return Rx, tot[36:].copy()

    # -- row-band building blocks (intra-frame sharding, wm.h wm_band_*; orchestration in bands.py) --------------
    def gram_totals(self, image):
        """the 44 Gram sums of `image` (of the owned rows in band mode) as a float64 array"""
        import torch
        pimg = plane_of(image, 1)
        buf = (C.c_double * (44 * pimg.frames))()
        torch.cuda.current_stream().synchronize()
        self._chk(lib().wm_gram(self._ctx, C.byref(pimg), buf, 0))
        return np.array(buf[:], dtype=np.float64)

    def band_configure(self, own_lo, own_hi, rows_global):
        self._chk(lib().wm_band_configure(self._ctx, int(own_lo), int(own_hi), int(rows_global)))

    def band_solve(self, totals):
        t = np.ascontiguousarray(totals, dtype=np.float64)
        st = (C.c_int * 1)()
        self._chk(lib().wm_band_solve(self._ctx, t.ctypes.data_as(_P(C.c_double)), 1, st, 0))
        return st[0]

    def band_stats(self, image, maskType):
        import torch
        pimg = plane_of(image, 1)
        out = (C.c_double * 2)()
        torch.cuda.current_stream().synchronize()
        self._chk(lib().wm_band_stats(self._ctx, int(maskType), C.byref(pimg), out, 0))
        return out[0], out[1]

    def band_embed(self, image, base, out, maskType, max_e, ss):
        import torch
        pin, pbase, pout = self._embed_planes(image, base, out)
        ms = (C.c_double * 2)(max_e, ss)
        a = (C.c_float * 1)()
        torch.cuda.current_stream().synchronize()
        self._chk(lib().wm_band_embed(self._ctx, int(maskType), C.byref(pin), C.byref(pbase), C.byref(pout), ms, a, 0))
        return a[0]

    def band_detect_sums(self, image, maskType):
        import torch
        pimg = plane_of(image, 1)
        out = (C.c_double * 3)()
        torch.cuda.current_stream().synchronize()
        self._chk(lib().wm_band_detect_sums(self._ctx, int(maskType), C.byref(pimg), out, 0))
        return out[0], out[1], out[2]

    # -- the same with the exchange resident in device memory (wm.h wm_band_*_dev): device tensors in, nothing synchronises.
    # The slot runs on torch's current stream (set_stream_current), so torch.distributed collectives order with the sweeps
    def set_stream_current(self, slot=0):
        import torch
        # torch's default stream has the handle 0, which wm_set_stream reads as "back to the slot's own stream": name the legacy
        # default stream by HIP's handle for it (hipStreamLegacy = 1)
        h = torch.cuda.current_stream().cuda_stream
        self._chk(lib().wm_set_stream(self._ctx, slot, C.c_void_p(h if h else 1)))

    def band_gram_dev(self, image, totals):
        """totals: float64 CUDA tensor [44] (one frame): receives this band's Gram sums"""
        pimg = plane_of(image, 1)
        self._chk(lib().wm_band_gram_dev(self._ctx, C.byref(pimg), C.c_void_p(totals.data_ptr()), 0))

    def band_solve_dev(self, totals):
        self._chk(lib().wm_band_solve_dev(self._ctx, C.c_void_p(totals.data_ptr()), 1, 0))

    def band_stats_dev(self, image, maskType, max_sum):
        pimg = plane_of(image, 1)
        self._chk(lib().wm_band_stats_dev(self._ctx, int(maskType), C.byref(pimg), C.c_void_p(max_sum.data_ptr()), 0))

    def band_embed_dev(self, image, base, out, maskType, gathered, nparts, a_dev):
        pin, pbase, pout = self._embed_planes(image, base, out)
        self._chk(lib().wm_band_embed_dev(self._ctx, int(maskType), C.byref(pin), C.byref(pbase), C.byref(pout), C.c_void_p(gathered.data_ptr()), nparts,
                                                C.c_void_p(a_dev.data_ptr()), 0))

    def band_detect_sums_dev(self, image, maskType, sums):
        pimg = plane_of(image, 1)
        self._chk(lib().wm_band_detect_sums_dev(self._ctx, int(maskType), C.byref(pimg), C.c_void_p(sums.data_ptr()), 0))

    def band_corr_dev(self, sums, corr):
        self._chk(lib().wm_band_corr_dev(self._ctx, C.c_void_p(sums.data_ptr()), 1, C.c_void_p(corr.data_ptr()), 0))

    # -- profiling ----------------------------------------------------------------------------
    def prof_enable(self, on=True):
        lib().wm_prof_enable(self._ctx, 1 if on else 0)

    def prof_reset(self):
        lib().wm_prof_reset(self._ctx)

    def prof_report(self):
        """{kernel name: (launches, total ms)} measured with hipEvents on the launch stream"""
        out = {}
        L = lib()
        for k in range(L.wm_prof_kernel_count()):
            n = C.c_uint64()
            ms = C.c_double()
            L.wm_prof_get(self._ctx, k, C.byref(n), C.byref(ms))
            if n.value:
                out[L.wm_prof_kernel_name(k).decode()] = (n.value, ms.value)
        return out
