"""The filter line search of the four solvers, without a GPU.

The batch driver behind idocp_*_update_solution(..., line_search = 1) (idocp_amd/csrc/line_search_filter.hpp: one filter per instance, every probe
evaluates the whole batch) is held by a stand-alone program under the address and undefined-behaviour sanitizers to a scalar restatement of
LineSearch::computeStepSize over LineSearchFilter, run once per instance (tests/cpp/line_search_filter.cpp): instances that stop at different
probes, steps at the minimum, mixed and filled filters, a dominating point, a failing evaluation."""
import os
import re
import subprocess

from helpers import ROOT

CSRC = os.path.join(ROOT, "idocp_amd", "csrc")


def test_batched_filter_line_search_against_the_scalar_loop_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "line_search_filter")
    r = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                        "-I" + CSRC, os.path.join(ROOT, "tests/cpp/line_search_filter.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "line search filter: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert "FAILED" not in r.stdout
    assert len(re.findall(r"^case ", r.stdout, flags=re.M)) == 15, r.stdout
