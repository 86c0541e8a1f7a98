"""tools/benchlib.py, the module the timing tools share, without a device: the alternation's call order, the wall clock's arithmetic on
a scripted clock, the library override in a child process, and that every tool starts and has given up its private copies."""
import ast
import json
import os
import py_compile
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)
import benchlib as bl  # noqa: E402

BENCHES = ("bits_bench", "convert_bench", "convert16_bench", "embed_keys_bench", "keys_bench", "keys_tiles_bench", "multi_bench", "offsets_bench",
           "quality_bench", "select_bench", "tiles_bench")
SCRIPTS = BENCHES + ("quick_bench", "ab")


def logging_routes(log, names=("a", "b", "c")):
    return {n: (lambda n=n: log.append(("run", n))) for n in names}


def test_alternate_warms_first_then_measures_every_route_once_per_round_in_order():
    log = []
    routes = logging_routes(log)
    count = {"n": 0}

    def measure(fn, iters):
        name = next(n for n, f in routes.items() if f is fn)
        log.append(("measure", name, iters))
        count["n"] += 1
        return count["n"]

    out = bl.alternate(routes, 3, 7, measure, warm=2)
    assert log == [("run", n) for _ in range(2) for n in "abc"] + [("measure", n, 7) for _ in range(3) for n in "abc"]
    assert out == {"a": [1, 4, 7], "b": [2, 5, 8], "c": [3, 6, 9]}
    assert list(out) == ["a", "b", "c"]


def test_alternate_skips_a_missing_route_everywhere():
    log = []
    routes = logging_routes(log)
    routes["b"] = None
    out = bl.alternate(routes, 2, 1, lambda fn, iters: fn(), warm=1)
    assert log == [("run", n) for _ in range(3) for n in "ac"]
    assert out == {"a": [None, None], "c": [None, None]}
    assert bl.alternate(logging_routes([]), 0, 1, lambda fn, iters: 0, warm=0) == {"a": [], "b": [], "c": []}


def test_wall_median_us_on_a_scripted_clock(monkeypatch):
    now = {"t": 100.0}
    monkeypatch.setattr(bl.time, "perf_counter", lambda: now["t"])
    seconds = iter([9.0, 9.0, 5e-6, 1e-6, 3e-6, 100e-6, 2e-6])  # two warm-up calls, then five timed ones
    calls = []

    def fn():
        calls.append(now["t"])
        now["t"] += next(seconds)

    got = bl.wall_median_us(fn, 5, warmup=2)
    assert len(calls) == 7
    assert got == pytest.approx(3.0, rel=1e-6)  # microseconds; the 9 s warm-up calls are not in it
    now["t"] = 0.0
    seconds = iter([1e-3, 3e-3])
    assert bl.wall_median_us(fn, 2) == pytest.approx(2000.0, rel=1e-9)  # an even count: the mean of the middle two


def test_median_of_rounds():
    assert bl.median_of_rounds([3.0, 1.0, 10.0]) == 2.0 + 1.0
    assert bl.median_of_rounds([4.0, 1.0, 2.0, 100.0]) == 3.0
    assert bl.median_of_rounds([5]) == 5.0 and isinstance(bl.median_of_rounds([5]), float)


LOAD = """
import json, sys
sys.path.insert(0, %r)
import benchlib
wm, synth = benchlib.load()
print("LOADED " + json.dumps({"lib": wm.LIB_PATH, "abi": [e[0] for e in wm.ABI], "synth": hasattr(synth, "synth_frame")}))
""" % TOOLS


def load_in_child(env):
    p = subprocess.run([sys.executable, "-c", LOAD], env=env, capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    return json.loads(next(l for l in p.stdout.splitlines() if l.startswith("LOADED "))[7:])


def test_load_points_at_the_other_build_and_trims_the_abi(tmp_path, wm):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "the host compiler that builds the oracle"
    src, so = tmp_path / "stub.c", tmp_path / "libwm_stub.so"
    src.write_text("int wm_device_count(void) { return 0; }\nconst char *wm_version(void) { return \"stub\"; }\n")
    subprocess.check_call([cc, "-shared", "-fPIC", "-o", str(so), str(src)])
    env = dict(os.environ, WM_AB_LIB=str(so))
    got = load_in_child(env)
    assert got["lib"] == str(so) and got["synth"]
    assert sorted(got["abi"]) == ["wm_device_count", "wm_version"]
    del env["WM_AB_LIB"]
    got = load_in_child(env)
    assert got["lib"] == wm.LIB_PATH == os.path.join(ROOT, "watermarking-gpu_amd", "libwm_hip.so")
    assert got["abi"] == [e[0] for e in wm.ABI] and len(got["abi"]) > 90


@pytest.mark.parametrize("script", SCRIPTS)
def test_every_script_starts_without_a_device(script, tmp_path):
    path = os.path.join(TOOLS, script + ".py")
    if script == "ab":  # no parser: its module body runs the children
        py_compile.compile(path, doraise=True, cfile=str(tmp_path / "ab.pyc"))
        return
    env = {k: v for k, v in os.environ.items() if k != "WM_AB_LIB"}
    p = subprocess.run([sys.executable, path, "--help"], env=env, capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr


def test_no_tool_keeps_a_private_copy():
    gone = {"round_median_us", "median_us", "device_span_us", "membench_us", "membench_gbs", "wall_us", "prof"}
    for script in SCRIPTS:
        tree = ast.parse(open(os.path.join(TOOLS, script + ".py")).read())
        defined = {n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef))}
        defined |= {n.id for n in ast.walk(tree) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store)}
        assert not defined & gone, (script, defined & gone)
        imports = {a.name for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom)) for a in n.names} | \
                  {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
        assert "benchlib" in imports, script
