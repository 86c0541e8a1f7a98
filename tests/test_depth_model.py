"""The numpy model of d-bit samples (tests/depth_model.py) holds what wm.h promises of the arithmetic itself: the exhaustive round
trip, full scale on exactly 255.0f, rounding ties to even, the clamps -- and wm_depth_scale returns the model's constants.  No GPU:
wm_depth_scale is pure host arithmetic."""
import ctypes as C

import numpy as np
import pytest

import depth_model as D

ALL = np.arange(65536, dtype=np.uint16)


@pytest.mark.parametrize("bits", D.BITS)
def test_round_trip_is_exact(bits):
    m = D.maxv(bits)
    v = ALL[: m + 1]
    g = D.unpack(v, bits)
    assert (D.pack(g, bits) == v).all()
    assert g[0] == 0.0 and g[-1] == np.float32(255.0) and (np.diff(g) > 0).all()
    # how far t = g * k_out lies from the code it rounds to: nowhere near a tie (the issue's figure: 0.004 at d = 16)
    t = (g * D.scale(bits)[1]).astype(np.float32)
    assert float(np.abs(t.astype(np.float64) - v).max()) <= 0.004


@pytest.mark.parametrize("bits", D.BITS)
def test_codes_above_full_scale_and_msb_alignment(bits):
    m, sh = D.maxv(bits), 16 - bits
    assert (D.unpack(ALL, bits) == D.unpack(np.minimum(ALL, m).astype(np.uint16), bits)).all()
    assert (D.pack(D.unpack(ALL, bits), bits) == np.minimum(ALL, m)).all()
    assert (D.unpack(ALL, bits, True) == D.unpack((ALL >> sh).astype(np.uint16), bits)).all()
    assert (D.pack(D.unpack(ALL, bits, True), bits, True) == (ALL >> sh) << sh).all()


@pytest.mark.parametrize("bits", D.BITS)
def test_ties_go_to_even_and_the_clamps(bits):
    g, k = D.tie_inputs(bits)
    assert (k % 2 == 0).any() and (k % 2 == 1).any()
    assert ((g * D.scale(bits)[1]).astype(np.float32) == (k + 0.5).astype(np.float32)).all()
    want = np.where(k % 2 == 0, k, k + 1)
    assert (D.pack(g, bits) == want).all()
    m = D.maxv(bits)
    special = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 255.0, np.nextafter(np.float32(255), np.float32(np.inf)), 1e9], np.float32)
    assert D.pack(special, bits).tolist() == [0, m, 0, 0, 0, m, m, m]


def test_depth_scale_is_the_models(wm):
    L = wm.lib()
    a, b = C.c_float(), C.c_float()
    for bits in D.BITS:
        assert L.wm_depth_scale(bits, C.byref(a), C.byref(b)) == wm.WM_OK
        k_in, k_out = D.scale(bits)
        assert np.float32(a.value).tobytes() == k_in.tobytes() and np.float32(b.value).tobytes() == k_out.tobytes()
        assert wm.depth_scale(bits) == (float(k_in), float(k_out))
    for bits in (8, 17, 0, -1):
        assert L.wm_depth_scale(bits, C.byref(a), C.byref(b)) == wm.WM_ERR_BAD_ARG
    assert L.wm_depth_scale(10, None, C.byref(b)) == wm.WM_ERR_BAD_ARG
    with pytest.raises(RuntimeError):
        wm.depth_scale(8)
