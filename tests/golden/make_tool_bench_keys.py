"""Records tests/golden/tool_bench_keys.json: for every tools/*_bench.py the sorted key paths of the JSON it writes when run with the
arguments of tests/test_gpu_tool_benches.py.  Run on a box with an MI355X and a built library, with the tools of the commit whose
output is the yardstick (the fixture in the repository: the commit before tools/benchlib.py):
    python tests/golden/make_tool_bench_keys.py [--tools DIR] [--out FILE]
DIR is a tools/ directory inside a checkout of that commit (default: this tree's).  Prints the seconds each tool took: three times
that is the test's time limit."""
import argparse
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_gpu_tool_benches as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tools", default=os.path.join(T.ROOT, "tools"))
    ap.add_argument("--out", default=T.FIXTURE)
    a = ap.parse_args()
    keys, took = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for tool in sorted(T.CASES):
            t0 = time.perf_counter()
            _, res = T.run_tool(os.path.abspath(a.tools), tool, os.path.join(tmp, tool + ".json"))
            took[tool] = round(time.perf_counter() - t0, 1)
            keys[tool] = sorted(T.key_paths(res))
            print(tool, took[tool], "s,", len(keys[tool]), "key paths", flush=True)
    with open(a.out, "w") as f:
        json.dump(keys, f, indent=1)
        f.write("\n")
    print("seconds: " + json.dumps(took))


if __name__ == "__main__":
    main()
