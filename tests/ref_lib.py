"""ctypes loader for oracle/_ref/libwm_ref.so: the reference's own OpenCL C kernels run on the CPU (oracle/build_ref.py,
oracle/clrt.c).  Test infrastructure only.

Variants: MAD = the reference's build options (-cl-mad-enable, main.cpp:106-108), STRICT = -ffp-contract=off.
"""
import ctypes as C
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
LIB_PATH = os.path.join(REF_DIR, "libwm_ref.so")
MANIFEST_PATH = os.path.join(REF_DIR, "MANIFEST.json")
MAD, STRICT = 0, 1
_LIB = None


def available():
    return os.path.exists(LIB_PATH) and os.path.exists(MANIFEST_PATH)


def reference_tree():
    """the reference checkout build_ref.py reads (REF, else beside the repository), or None when it is absent"""
    ref = os.environ.get("REF") or os.path.join(os.path.dirname(ROOT), "reference")
    files = [os.path.join(ref, "Watermark_GPU", "kernels", h) for h in ("nvf.hpp", "me_p3.hpp", "scaled_neighbors_p3.hpp")]
    files.append(os.path.join(ref, "Watermark_GPU", "Watermark.hpp"))
    return ref if all(os.path.isfile(f) and os.access(f, os.R_OK) for f in files) else None


def manifest():
    with open(MANIFEST_PATH) as f:
        return json.load(f)


def manifest_sources_text():
    """the sha256 of every extracted reference source, as one canonical string (recorded in the fixture)"""
    return json.dumps(manifest()["sources"], sort_keys=True)


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(LIB_PATH)
        fp = C.POINTER(C.c_float)
        L.wmref_nvf.argtypes = [C.c_int, C.c_int, fp, C.c_int, C.c_int, fp]
        L.wmref_scaled_neighbors.argtypes = [C.c_int, fp, C.c_int, C.c_int, fp, fp]
        L.wmref_me_partials.argtypes = [C.c_int, fp, C.c_int, C.c_int, fp, fp]
        _LIB = L
    return _LIB


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _c32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def nvf(x, p=3, variant=MAD):
    """the nvf kernel (nvf.hpp, -Dp=p) on a row-major plane; returns the row-major mask"""
    x = _c32(x)
    out = np.empty_like(x)
    assert lib().wmref_nvf(variant, p, _f(x), x.shape[0], x.shape[1], _f(out)) == 0
    return out


def scaled_neighbors(x, c, variant=MAD):
    """the scaled_neighbors_p3 kernel with coefficients c[8]; returns the row-major plane"""
    x = _c32(x)
    c = _c32(c)
    assert c.shape == (8,)
    out = np.empty_like(x)
    assert lib().wmref_scaled_neighbors(variant, _f(x), x.shape[0], x.shape[1], _f(c), _f(out)) == 0
    return out


def me_partials(x, variant=MAD):
    """the me kernel's raw outputs: RxPartial [rows, ALIGN64(cols)] and rxPartial [rows, ALIGN64(cols) / 8], as written"""
    x = _c32(x)
    rows, cols = x.shape
    pw = (cols + 63) // 64 * 64
    Rp = np.full((rows, pw), np.nan, np.float32)
    rp = np.full((rows, pw // 8), np.nan, np.float32)
    assert lib().wmref_me_partials(variant, _f(x), rows, cols, _f(Rp), _f(rp)) == 0
    return Rp, rp


def gram_partials(x, variant=MAD):
    """per work-group sums [rows * ngroups, 44] in the oracle's order (36 upper-triangle Rx sums, row-major, then the 8
    rx sums), read off me_partials: work-group g of row r wrote Rx sum RxMappings[l] at lane l and the rx sums at lanes
    0-7 of its rx block (me_p3.hpp:61-82)"""
    Rp, rp = me_partials(x, variant)
    rows, pw = Rp.shape
    ng = pw // 64
    R = Rp.reshape(rows * ng, 8, 8)
    iu = np.triu_indices(8)
    return np.concatenate([R[:, iu[0], iu[1]], rp.reshape(rows * ng, 8)], axis=1)
