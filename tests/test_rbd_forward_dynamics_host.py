"""Forward dynamics (idocp_rbd_forward_dynamics_batch, idocp_rbd_rollout) without a GPU: the ctypes mirror of idocp_rbd_fd_io_t against the header,
the facade's additions compile, and the argument checks that need no device."""
import ctypes as C
import os
import subprocess

from helpers import ROOT
from idocp_amd import capi

E_ARG = -1
INCLUDE = os.path.join(ROOT, "include")

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "idocp_hip.h"
#define FIELD(name) printf(#name " %zu %zu\n", offsetof(idocp_rbd_fd_io_t, name), sizeof(((idocp_rbd_fd_io_t*)0)->name))
int main(void) {
  printf("sizeof %zu\n", sizeof(idocp_rbd_fd_io_t));
  FIELD(q); FIELD(v); FIELD(u); FIELD(contact_points); FIELD(a); FIELD(f); FIELD(q_next); FIELD(v_next);
  return 0;
}
"""


def test_ctypes_mirror_matches_the_header(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    r = subprocess.run(["gcc", "-std=c99", "-I" + INCLUDE, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert int(lines[0].split()[1]) == C.sizeof(capi.RbdFdIO)
    fields = [x.split() for x in lines[1:] if x]
    assert [x[0] for x in fields] == [name for name, _ in capi.RbdFdIO._fields_]      # (the order of the struct)
    for name, offset, size in fields:
        d = getattr(capi.RbdFdIO, name)
        assert (d.offset, d.size) == (int(offset), int(size)), name
    # idocp_rbd_io_t is what it was: 14 pointers
    assert C.sizeof(capi.RbdIO) == 14 * C.sizeof(C.c_void_p)


def test_null_handle_is_an_argument_error():
    lib = capi.lib()
    io = capi.RbdFdIO()
    act = (C.c_int * 4)(1, 1, 1, 1)
    for fn in (lib.idocp_rbd_forward_dynamics_batch, lib.idocp_rbd_forward_dynamics_batch_device):
        assert fn(None, capi.RBD_STAGE, 1, act, 0.05, 0.01, C.byref(io)) == E_ARG
        assert b"idocp_rbd_forward_dynamics_batch" in lib.idocp_last_error()
    for fn in (lib.idocp_rbd_rollout, lib.idocp_rbd_rollout_device):
        assert fn(None, 1, 1, act, 0.05, 0.01, None, None, None, None, None, None, 1) == E_ARG
        assert b"idocp_rbd_rollout" in lib.idocp_last_error()


def test_facade_additions_compile_without_gpu(tmp_path):
    exe = str(tmp_path / "forward_dynamics_surface")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + INCLUDE, os.path.join(ROOT, "tests/cpp/forward_dynamics_surface.cpp"),
                        "-L" + os.path.join(ROOT, "idocp_amd/lib"), "-lidocp_hip", "-Wl,-rpath," + os.path.join(ROOT, "idocp_amd/lib"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "forward dynamics surface: ok" in r.stdout, r.stdout + r.stderr
