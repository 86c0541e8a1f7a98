"""CPU tests of the key-bank surface (wm.h wm_keys_*, wm_detect_keys): every symbol is exported and bound, and argument
errors come back before any device is touched (no GPU needed)."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_SYMBOLS = ("wm_keys_create", "wm_keys_destroy", "wm_keys_count", "wm_keys_rows", "wm_keys_cols", "wm_keys_device_ptr",
               "wm_keys_set", "wm_keys_load_file", "wm_keys_generate", "wm_detect_keys")


@pytest.fixture(scope="module")
def L(wm):
    return wm.lib()


def test_key_symbols_declared_exported_and_bound(L, wm):
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    bound = {name for name, _, _ in wm.ABI}
    for s in KEY_SYMBOLS:
        assert s + "(" in hdr, s
        assert hasattr(L, s), s
        assert s in bound, s
    assert "#define WM_KEYS_MAX 4096" in hdr and wm.WM_KEYS_MAX == 4096


def test_keys_create_argument_errors(L, wm):
    k = C.c_void_p(123)
    assert L.wm_keys_create(None, 0, 8, 8, 2) == wm.WM_ERR_BAD_ARG
    for rows, cols, n in ((0, 8, 2), (8, 0, 2), (-1, 8, 2), (8, 8, 0), (8, 8, -3), (8, 8, wm.WM_KEYS_MAX + 1), (32769, 8, 1)):
        assert L.wm_keys_create(C.byref(k), 0, rows, cols, n) == wm.WM_ERR_BAD_ARG, (rows, cols, n)
        assert not k.value  # *out is cleared


def test_keys_calls_on_null_bank(L, wm):
    w = np.zeros(64, np.float32)
    assert L.wm_keys_set(None, 0, w.ctypes.data_as(C.c_void_p), wm.WM_MEM_HOST) == wm.WM_ERR_BAD_ARG
    assert L.wm_keys_load_file(None, 0, b"/nonexistent") == wm.WM_ERR_BAD_ARG
    assert L.wm_keys_generate(None, 0, 1) == wm.WM_ERR_BAD_ARG
    assert L.wm_keys_count(None) == 0 and L.wm_keys_rows(None) == 0 and L.wm_keys_cols(None) == 0
    assert not L.wm_keys_device_ptr(None, 0)
    L.wm_keys_destroy(None)  # no-op


def test_detect_keys_argument_errors(L, wm):
    plane = wm.wm_plane(None, 8, 8, 1, wm.WM_F32, wm.WM_MEM_DEVICE, 1, 8, 0, 0)
    corr = (C.c_float * 4)()
    assert L.wm_detect_keys(None, 0, C.byref(plane), None, corr, None, wm.WM_SLOT_SYNC) == wm.WM_ERR_BAD_ARG


def test_keys_python_surface(wm):
    assert hasattr(wm, "KeySet") and hasattr(wm.Watermark, "detectKeys") and hasattr(wm.Watermark, "detect_keys_async")
    for m in ("from_seeds", "from_files", "set", "close"):
        assert hasattr(wm.KeySet, m), m
    with pytest.raises(RuntimeError):
        wm.KeySet(8, 8, 0)
    with pytest.raises(RuntimeError):
        wm.KeySet(0, 8, 1)


def _has_device(L):
    return L.wm_device_count() > 0


def test_w_file_errors(L, wm, tmp_path):
    """wm_create_from_file's checks and codes (Watermark.cpp:62-75): a missing file is WM_ERR_W_OPEN, a wrong size WM_ERR_W_SIZE.
    A bank needs a device.  Without one, this test checks that wm_keys_create reports that only after its argument checks
    (tests/test_gpu_keys.py checks the file codes on the GPU)."""
    bad = tmp_path / "w_wrong.dat"
    np.zeros(10, np.float32).tofile(bad)
    k = C.c_void_p()
    rc = L.wm_keys_create(C.byref(k), 0, 4, 4, 2)
    if rc == wm.WM_ERR_NO_DEVICE:
        assert not _has_device(L)
        # the argument checks still come first
        assert L.wm_keys_create(C.byref(k), 0, 4, 4, 0) == wm.WM_ERR_BAD_ARG
        return
    assert rc == wm.WM_OK
    try:
        assert L.wm_keys_load_file(k, 0, str(tmp_path / "missing.dat").encode()) == wm.WM_ERR_W_OPEN
        assert L.wm_keys_load_file(k, 0, str(bad).encode()) == wm.WM_ERR_W_SIZE
        assert L.wm_keys_load_file(k, 2, str(bad).encode()) == wm.WM_ERR_BAD_ARG
        assert L.wm_keys_load_file(k, -1, str(bad).encode()) == wm.WM_ERR_BAD_ARG
        assert L.wm_keys_load_file(k, 0, None) == wm.WM_ERR_BAD_ARG
        assert L.wm_keys_set(k, 0, None, wm.WM_MEM_HOST) == wm.WM_ERR_BAD_ARG
        assert L.wm_keys_generate(k, 5, 1) == wm.WM_ERR_BAD_ARG
    finally:
        L.wm_keys_destroy(k)
