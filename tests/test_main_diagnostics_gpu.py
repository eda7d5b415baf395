"""main.py --diagnostics on the MI355X, as a child process: the diagnostics ride beside the --analysis analyzer and their
JSON agrees with what the analyzer prints.  What a run without --diagnostics prints is checked against the run with
them, in the same build: it has no diagnostics line, and its lines are, in order, the lines the other run prints around
its diagnostics.  (That the output equals the previous commit's byte for byte was checked once, by running that
commit's driver beside this one; no transcript is committed, because the printed loss depends on the device.)"""
import json
import os
import re
import subprocess
import sys

import pytest

import nbdt_path

pytestmark = pytest.mark.gpu

MAIN = os.path.join(nbdt_path.PKG_DIR, "main.py")
COMMON = ("--eval --synthetic 256 --arch ResNet18 --dataset CIFAR10 --batch-size 64 --seed 3 "
          "--analysis HardEmbeddedDecisionRules").split()


def _run(cwd, extra):
    out = subprocess.run([sys.executable, MAIN] + COMMON + extra, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def test_diagnostics_ride_beside_the_analyzer(tmp_path):
    plain = _run(tmp_path, [])
    with_diag = _run(tmp_path, ["--diagnostics", "TreeStatistics", "ConfusionMatrix", "--diagnostics-out", "f.json"])
    report = json.loads((tmp_path / "f.json").read_text())
    assert set(report) == {"TreeStatistics", "ConfusionMatrix"}
    stats = report["TreeStatistics"]
    printed = re.search(r"NBDT-Hard: ([0-9.]+)%", with_diag)
    hits = re.search(r"\[NBDT-Hard\] rules accuracy ([0-9.]+)% \((\d+) of (\d+)\)", with_diag)
    assert printed and hits
    assert stats["totals"][0] == int(hits.group(3)) and stats["totals"][2] == int(hits.group(2))
    assert "%.3f" % stats["accuracy"]["hard"] == printed.group(1)
    backbone = re.search(r"\| Acc: ([0-9.]+)%", with_diag)
    assert "%.3f" % stats["accuracy"]["net"] == backbone.group(1)
    matrix = report["ConfusionMatrix"]["matrix"]
    assert report["ConfusionMatrix"]["kind"] == "net" and sum(map(sum, matrix)) == stats["totals"][0]
    assert sum(matrix[i][i] for i in range(10)) == stats["totals"][1]
    assert sum(stats["first_error_depth"]) == stats["totals"][0] and len(stats["nodes"]) == 9
    assert "[TreeStatistics]" in with_diag and "(diagonal)" in with_diag
    # without the flag: no diagnostics line, and exactly the lines the other run prints around its diagnostics
    assert "[TreeStatistics]" not in plain and "(diagonal)" not in plain
    rest = iter(with_diag.splitlines())
    assert all(any(line == other for other in rest) for line in plain.splitlines()), (plain, with_diag)
