"""The ragged-item cursor and launch rule of the persistent decoder kernels (mimic3_amd/csrc/items.h), proved by brute force on the CPU.

tests/emu/item_cursor_check.cpp is a stand-alone program: it is compiled here with g++ against items.h (the CPU model's side of the
header, -DMI355_EMU) and the host half in launch_util.cpp, with the address and undefined-behaviour sanitizers, and run once.  For
every item width in {31, 32, 127, 128}, extra in {0, 1}, T in {1, N - 1, N, N + 1, 260}, length tables of 1 .. 9 rows drawn from
{0, 1, N - 1, N, N + 1, T - 1, T, T + 5} (empty rows first, in the middle and last; all rows empty; lengths above T) and grids
W = 1 .. 24, 32, 100, 256 it lists the items (b, t0, len, last) row by row and checks that

  * the grid-stride walk w, w + W, ... through decode(), in the order the host rule grants a request for XCD-major, and
  * k_mrf_p's walk (groups of min(W, 8), contiguous eighths, stride = the group's workgroups)

each visit every listed item exactly once with exactly those fields, that the remapped indices of a workgroup strictly increase
wherever the rule grants XCD-major, and that the host's count agrees with the list.  The kernel-level tests can afford a handful of
grids; a kernel that adopts the cursor inherits this.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_item_cursor_visits_every_item_once_on_every_grid(tmp_path):
    exe = tmp_path / "item_cursor_check"
    csrc = os.path.join(ROOT, "mimic3_amd", "csrc")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Og", "-DMI355_EMU", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wno-psabi", "-Wno-unused-function", "-I", emu, "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(emu, "item_cursor_check.cpp"), os.path.join(csrc, "launch_util.cpp"), "-o", str(exe), "-lpthread"], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert " 0 failures" in p.stdout
