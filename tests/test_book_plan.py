"""Vanilla books on the host (no GPU): the chunk rule csrc/mc_launch_shape.hpp: book_plan, and the layout of the book entry structs."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_book_plan_rules(tmp_path):
    """book_plan (hipcc, host code only, nothing launched; tests/cpp/book_plan_check.hip): every unit of every entry covered exactly
    once, no chunk across a multiple of 2^32 units, an entry's chunks the same when it moves to index 4000, when the book is shuffled
    or other entries are added, masks on the edge chunks only, bounded arrivals on every ticket word (a 1e10-path entry included),
    and the single call's refusals with the index of the first bad entry."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    exe = tmp_path / "book_plan_check"
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "montecarlocuda_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "book_plan_check.hip"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all book_plan checks passed" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


def test_book_entry_layout(tmp_path):
    """sizeof and offsetof of mc_book_entry_f32 / _f64, compiled from include/mc_mi355x.h, against the ctypes mirror in _lib.py."""
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "mc_mi355x.h"
#define P(T) printf("%s %zu %zu %zu %zu %zu\\n", #T, sizeof(T), offsetof(T, option), offsetof(T, seed), offsetof(T, first_path), offsetof(T, n_paths))
int main(void) { P(mc_book_entry_f32); P(mc_book_entry_f64); printf("MC_MAX_BOOK %d\\n", MC_MAX_BOOK); return 0; }
""")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    from montecarlocuda_amd import _lib
    for X in ("f32", "f64"):
        S = _lib.BOOK_ENTRY[X]
        assert got[f"mc_book_entry_{X}"] == [C.sizeof(S), S.option.offset, S.seed.offset, S.first_path.offset, S.n_paths.offset], X
    assert got["MC_MAX_BOOK"] == [_lib.MAX_BOOK]
