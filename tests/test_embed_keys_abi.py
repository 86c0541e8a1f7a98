"""CPU tests of wm_embed_keys (wm.h): the symbol is declared, exported and bound, argument errors come back before any device
is touched, and the Python surface checks the shapes it is handed (no GPU needed)."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L(wm):
    return wm.lib()


def test_embed_keys_declared_exported_and_bound(L, wm):
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert "int wm_embed_keys(" in hdr
    assert hasattr(L, "wm_embed_keys")
    assert "wm_embed_keys" in {name for name, _, _ in wm.ABI}
    assert "makeWatermarkKeys(" in open(os.path.join(ROOT, "include", "Watermark.hpp")).read()


def test_embed_keys_kernel_names(L, wm):
    names = {L.wm_prof_kernel_name(k).decode() for k in range(L.wm_prof_kernel_count())}
    assert {"k_stats_keys", "k_embed_keys_fold", "k_embed_keys"} <= names


def _planes(wm, frames=1, nkeys=2):
    gray = wm.wm_plane(None, 8, 8, 1, wm.WM_F32, wm.WM_MEM_DEVICE, frames, 8, 0, 64)
    out = wm.wm_plane(None, 8, 8, 1, wm.WM_F32, wm.WM_MEM_DEVICE, frames * nkeys, 8, 0, 64)
    return gray, out


@pytest.mark.parametrize("mask", [0, 1, 2, -1])
def test_embed_keys_null_context(L, wm, mask):
    """a null context is WM_ERR_BAD_ARG whatever the other arguments are (null keys, null out, any mask), and the call returns
    before it touches a device.  The checks that need a context -- a bad mask, ME with p != 3 (WM_ERR_BAD_P), a null bank or out,
    the output-side refusals -- are tests/test_gpu_embed_keys.py::test_refusals_and_capacity"""
    gray, out = _planes(wm)
    a = (C.c_float * 2)()
    st = (C.c_int * 1)()
    for keys in (None, C.c_void_p(1)):
        for o in (None, C.byref(out)):
            assert L.wm_embed_keys(None, mask, C.byref(gray), C.byref(gray), keys, o, a, st, wm.WM_SLOT_SYNC) == wm.WM_ERR_BAD_ARG
    assert L.wm_embed_keys(None, mask, None, None, None, None, None, None, 0) == wm.WM_ERR_BAD_ARG


def test_embed_keys_python_surface(wm):
    assert hasattr(wm.Watermark, "makeWatermarkKeys") and hasattr(wm.Watermark, "embed_keys_async")
    import inspect
    params = list(inspect.signature(wm.Watermark.makeWatermarkKeys).parameters)
    assert params == ["self", "inputImage", "outputImage", "keys", "maskType", "out"]
    params = list(inspect.signature(wm.Watermark.embed_keys_async).parameters)
    assert params[:7] == ["self", "inputImage", "outputImage", "out", "keys", "maskType", "slot"]


def test_embed_keys_python_rejects_cpu_tensors(wm):
    """planes must be GPU tensors (no CPU fallback): a CPU tensor is refused before the library is called"""
    torch = pytest.importorskip("torch")

    class _Keys:
        count = 2
        handle = None

    eng = object.__new__(wm.Watermark)
    eng._ctx = None
    x = torch.zeros(8, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.makeWatermarkKeys(x, x, _Keys(), wm.MASK_TYPE.ME)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.embed_keys_async(x, x, torch.zeros(2, 8, 8), _Keys(), wm.MASK_TYPE.ME, 0)
