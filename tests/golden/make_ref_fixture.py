"""Writes tests/golden/ref_kernels.npz: outputs of the reference's own kernels (the MAD build of oracle/_ref, see
oracle/build_ref.py) on a few small planes, so that tests/test_ref_kernels.py holds the oracle to them even where
oracle/_ref cannot be built.  Needs oracle/_ref:
    python oracle/build_ref.py && python tests/golden/make_ref_fixture.py

Keys: x_<plane>, c_<coefficient set>, nvf_<plane>_p<p>, sn_<plane>_<coefficient set>, part_<plane> (the me kernel's
work-group sums in the oracle's order), manifest_sources (the sha256 of the extracted reference sources).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402
import ref_lib as R  # noqa: E402
from conftest import load_pair  # noqa: E402


def main():
    assert R.available(), "oracle/_ref is not built"
    import json
    with open(os.path.join(HERE, "golden.json")) as f:
        golden = json.load(f)
    rng = np.random.default_rng(20261015)
    r, c = np.indices((16, 16))
    planes = {
        "u8": rng.integers(0, 256, (17, 33)).astype(np.float32),
        "f32": rng.uniform(0, 255, (15, 17)).astype(np.float32),
        "checker": (((r + c) & 1) * 255).astype(np.float32),
        "const": np.full((3, 3), 97.25, np.float32),
        "wide": rng.uniform(0, 255, (3, 129)).astype(np.float32),
        "crop": O.rgb2gray(load_pair(golden, "720p_crop")[0]),
    }
    coefs = {"solved": O.me_mask(planes["crop"])[1],
             "mixed": np.array([0.3333333, -1e-4, 12.5, -0.7071068, 1e-7, -255.0, 0.1, -3.14159], np.float32)}
    out = {"manifest_sources": np.array(R.manifest_sources_text())}
    for name, x in planes.items():
        out["x_" + name] = x
        for p in (3, 5, 7, 9):
            out[f"nvf_{name}_p{p}"] = R.nvf(x, p, R.MAD)
        for cname, cv in coefs.items():
            out[f"sn_{name}_{cname}"] = R.scaled_neighbors(x, cv, R.MAD)
        out["part_" + name] = R.gram_partials(x, R.MAD)
    for cname, cv in coefs.items():
        out["c_" + cname] = cv
    path = os.path.join(HERE, "ref_kernels.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
