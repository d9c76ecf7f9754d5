"""The kernel forms of an OCPSolver / ParNMPCSolver handle, without a GPU.

The rules that resolve a handle's record (idocp_amd/csrc/ocp_forms.hpp: side stream, fused forward sweep, wide backward sweep) are held by a
stand-alone program under the address and undefined-behaviour sanitizers to what the library chose before the record existed, and the
library's sources are held to reading the process environment in one place only (idocp_amd/csrc/host_util.hpp)."""
import glob
import os
import re
import subprocess

from helpers import ROOT

CSRC = os.path.join(ROOT, "idocp_amd", "csrc")


def test_forms_by_batch_size_and_forced_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "ocp_forms")
    r = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                        "-I" + CSRC, os.path.join(ROOT, "tests/cpp/ocp_forms.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ocp forms: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    rows = {int(b): (int(s), int(f), int(w)) for b, s, f, w in re.findall(r"forms (\d+): side (\d) fused (\d) wide (\d)", r.stdout)}
    assert rows == {1: (0, 0, 1), 16: (0, 0, 1), 17: (0, 0, 0), 127: (0, 0, 0), 128: (1, 0, 0), 191: (1, 0, 0), 192: (1, 1, 0), 1024: (1, 1, 0)}


def test_the_environment_is_read_in_one_place():
    hips = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    headers = sorted(glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert len(hips) >= 20 and len(headers) >= 20
    reads = lambda path: "getenv" in open(path).read()      # noqa: E731
    assert [os.path.basename(p) for p in hips if reads(p)] == []
    assert [os.path.basename(p) for p in headers if reads(p)] == ["host_util.hpp"]
