"""Every tools/*_bench.py runs once on the smallest work its own flags allow and writes the JSON it always wrote: the set of key
paths equals tests/golden/tool_bench_keys.json, which tests/golden/make_tool_bench_keys.py recorded from the tools as they stood
before they were moved onto tools/benchlib.py.  The four tools that used to ignore WM_AB_LIB run a second time against a copy of the
tree's library under another file name.

Time limits: three times what the tools took before the move, one run each with the arguments below on an MI355X (seconds, process
start and the torch import included):
  bits 2.4  convert16 3.1  convert 3.1  embed_keys 3.0  keys 2.5  keys_tiles 2.6  multi 3.0  offsets 2.5  quality 7.0  select 2.6  tiles 2.6
"""
import json
import os
import shutil
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "tool_bench_keys.json")

SMALL = ["--rows", "64", "--cols", "256", "--iters", "2"]
ROUNDS = ["--rounds", "2"]
# tool -> (arguments, seconds the tool took before the move); a dimension a tool has no flag for stays at its default
CASES = {
    "bits_bench": (SMALL + ROUNDS + ["--tile", "32x32", "--nbits", "8", "--frames", "1", "--masks", "0"], 2.4),
    "convert_bench": (SMALL + ROUNDS + ["--batch", "1"], 3.1),
    "convert16_bench": (SMALL + ROUNDS + ["--batch", "1"], 3.1),
    "embed_keys_bench": (SMALL + ["--keys", "1"], 3.0),
    "keys_bench": (SMALL + ["--keys", "1", "--frames", "1"], 2.5),
    "keys_tiles_bench": (SMALL + ROUNDS + ["--tile", "32x32", "--keys", "1", "--frames", "1"], 2.6),
    "multi_bench": (SMALL + ROUNDS + ["--tile", "32x32", "--copies", "1", "--masks", "0"], 3.0),
    "offsets_bench": (SMALL + ROUNDS + ["--rects", "1x4", "--frames", "1"], 2.5),
    "quality_bench": (SMALL + ROUNDS + ["--batch", "1", "--frames", "1"], 7.0),
    "select_bench": (SMALL + ROUNDS + ["--frames", "2", "--configs", "f32:ME"], 2.6),
    "tiles_bench": (SMALL + ROUNDS + ["--tile", "32x32", "--cases", "f32:1"], 2.6),
}
IGNORED_THE_OVERRIDE = ("convert_bench", "convert16_bench", "quality_bench", "select_bench")


def key_paths(obj, at=""):
    """the set of key paths of a JSON value: nested keys joined with "/", the elements of a list as "[]" """
    if isinstance(obj, dict):
        return set().union({at} if not obj else (), *(key_paths(v, at + "/" + k if at else k) for k, v in obj.items()))
    if isinstance(obj, list):
        return set().union({at + "[]"}, *(key_paths(v, at + "[]") for v in obj))
    return {at}


def run_tool(tools_dir, tool, out, env=None, limit=None):
    """one fresh child process, ended after `limit` seconds; returns (CompletedProcess, the JSON it wrote)"""
    args = CASES[tool][0]
    p = subprocess.run([sys.executable, os.path.join(tools_dir, tool + ".py")] + args + ["--json", out], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=limit)
    assert p.returncode == 0, p.stdout + p.stderr
    with open(out) as f:
        return p, json.load(f)


@pytest.mark.parametrize("tool", sorted(CASES))
def test_tool_writes_its_json(tool, tmp_path):
    with open(FIXTURE) as f:
        want = json.load(f)[tool]
    _, res = run_tool(os.path.join(ROOT, "tools"), tool, str(tmp_path / "out.json"), limit=3 * CASES[tool][1])
    assert sorted(key_paths(res)) == want


@pytest.mark.parametrize("tool", IGNORED_THE_OVERRIDE)
def test_tool_takes_the_library_override(tool, tmp_path, wm):
    """none of the four reports the library's name, so the run succeeding is the check: the copy binds, the call that the tool times
    exists in it, and no second HIP runtime hides the device from it"""
    copy = str(tmp_path / "libwm_elsewhere.so")
    shutil.copy(wm.LIB_PATH, copy)
    p, res = run_tool(os.path.join(ROOT, "tools"), tool, str(tmp_path / "out.json"), env=dict(os.environ, WM_AB_LIB=copy), limit=3 * CASES[tool][1])
    assert "no HIP device" not in p.stdout + p.stderr and "WM_ERR_NO_DEVICE" not in p.stdout + p.stderr
    assert res
