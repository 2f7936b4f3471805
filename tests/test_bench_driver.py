"""tools/_bench.py run_cases, the one parent side of every tools/bench_*.py: each case is a fresh child under `timeout -k 10`; a child that
fails or outlives its limit ends the run, no later case is started and nothing is appended.  The child here is a stand-in script that
drops a marker file per case: no GPU and no product library."""
import importlib.util
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CHILD = """import json, sys, time
from pathlib import Path
case, mode = sys.argv[1], sys.argv[2]
(Path(__file__).parent / ("started_" + case)).touch()
if mode == "fail" and case == "b":
    print("about to fail")
    sys.exit(3)
if mode == "hang" and case == "b":
    time.sleep(30)
print("a line that is not the result")
print(json.dumps({"case": case, "ms": 1.5}))
"""


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("_bench", ROOT / "tools" / "_bench.py")
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def run(bench, tmp_path, mode, **kwargs):
    child = tmp_path / "child.py"
    child.write_text(CHILD)
    out = tmp_path / "sub" / "out.jsonl"
    bench.run_cases("stand_in", ("a", "b", "c"), lambda case: [case, mode], 1, out, script=child, **kwargs)
    return out


def head_commit():
    try:
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def started(tmp_path):
    return sorted(p.name for p in tmp_path.glob("started_*"))


def test_every_case_succeeds(bench, tmp_path, capsys):
    out = run(bench, tmp_path, "ok", header={"steps": 2})
    lines = out.read_text().splitlines()
    assert len(lines) == 1 and capsys.readouterr().out.strip() == lines[0]
    result = json.loads(lines[0])
    assert list(result) == ["tool", "steps", "commit", "a", "b", "c"]
    assert result["tool"] == "stand_in" and result["steps"] == 2 and result["b"] == {"case": "b", "ms": 1.5}
    assert result["commit"] == head_commit()
    assert started(tmp_path) == ["started_a", "started_b", "started_c"]


def test_merged_results(bench, tmp_path):
    """the single-measurement form: the child's keys go into the top level"""
    result = json.loads(run(bench, tmp_path, "ok", merge=True).read_text())
    assert list(result) == ["tool", "commit", "case", "ms"]


@pytest.mark.parametrize("mode, status", [("fail", "exit status 3"), ("hang", "exit status 124")])
def test_a_failed_or_overdue_case_ends_the_run(bench, tmp_path, capsys, mode, status):
    with pytest.raises(SystemExit) as e:
        run(bench, tmp_path, mode)
    assert e.value.code not in (0, None)
    assert "case b" in str(e.value.code) and status in str(e.value.code) and "nothing more is started" in str(e.value.code)
    assert started(tmp_path) == ["started_a", "started_b"]  # c was never started
    assert not (tmp_path / "sub" / "out.jsonl").exists()
    if mode == "fail":
        assert "about to fail" in capsys.readouterr().err
