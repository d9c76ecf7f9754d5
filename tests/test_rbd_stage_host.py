"""The staging plan behind the host-pointer calls of the rigid-body API (idocp_amd/csrc/rbd_stage.hpp) without a GPU: tests/cpp/rbd_stage_layout.cpp
declares the slot sets of the five calls with every pattern of optional arrays and holds the layout to its rules (16-byte slots that do not
overlap, absent arrays without room, the exact upload / download lists, the zero fill of MJtJinv alone) as a stand-alone program under the address
and undefined-behaviour sanitizers."""
import os
import subprocess

from helpers import ROOT


def test_stage_layout_of_the_five_host_forms(tmp_path):
    exe = str(tmp_path / "rbd_stage_layout")
    r = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "idocp_amd/csrc"), os.path.join(ROOT, "tests/cpp/rbd_stage_layout.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "rbd stage layout: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
