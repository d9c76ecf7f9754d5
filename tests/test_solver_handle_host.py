"""What the four solver facades share (include/idocp/detail/solver_core.hpp), on the host: tests/cpp/solver_handle.cpp holds detail::OwnedHandle -- the owner
behind their copy and move -- to its clone / destroy bookkeeping on a stub handle type, compiled with g++ under the address and undefined-behaviour
sanitizers and run (neither the library nor a device is needed); and each of the four solver headers compiles on its own."""
import os
import subprocess

import pytest

from helpers import ROOT

EXE = os.path.join(ROOT, "tests", "cpp", "_build", "solver_handle")
INCLUDE = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Wshadow", "-Werror", "-fsanitize=address,undefined", "-I" + INCLUDE,
           os.path.join(ROOT, "tests", "cpp", "solver_handle.cpp"), "-o", EXE]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return EXE


def test_owner_special_members(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


def test_failed_clone_fails_the_reference_way(exe):
    r = subprocess.run([exe, "clone_fails"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "stub: clone refused" in r.stderr and "not reached" not in r.stdout, (r.returncode, r.stdout, r.stderr)


@pytest.mark.parametrize("header", ["idocp/ocp/ocp_solver.hpp", "idocp/ocp/parnmpc_solver.hpp", "idocp/unocp/unocp_solver.hpp", "idocp/unocp/unparnmpc_solver.hpp"])
def test_solver_header_is_self_contained(header, tmp_path):
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "%s"\n' % header)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", INCLUDE, str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
