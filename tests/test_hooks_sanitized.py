"""The hooks of include/mi355vits_lab.h under the address and undefined-behaviour sanitizers, on the CPU only.

Every kernel-level test reaches its kernel through these hooks (mimic3_amd/csrc/lab_api.cpp): a short buffer or a miscounted size there
is a wrong answer or a fault inside the test infrastructure.  tests/emu/hooks_check.cpp is a stand-alone program with its own main: it
is compiled here with the CPU model's sources (mimic3_amd.build's SOURCES + HOOK_SOURCES and tests/emu/hip_emu_impl.cpp, -DMI355_EMU),
all of them with -fsanitize=address,undefined, linked and run once.  The model's hipMalloc is malloc, so the sanitizer sees every byte a
hook or a kernel touches outside a "device" buffer.  The program checks HookScope itself and calls every device hook at the smallest
shape its kernel takes, every impl and math mode, every optional pointer given once and withheld once, then every hook that takes
lengths with a length of T + 1 (refused, nothing written).  Results are not compared: the kernel suites do that.
"""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

from mimic3_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_hook_runs_clean_under_the_sanitizers(tmp_path):
    emu = os.path.join(ROOT, "tests", "emu")
    cxx = os.environ.get("CXX", "g++")
    base = [cxx, "-std=c++17", "-Og", "-DMI355_EMU", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-psabi",
            "-Wno-unused-result", "-I", emu, "-I", os.path.join(ROOT, "include")]
    srcs = [os.path.join(build.CSRC, s) for s in build.SOURCES + build.HOOK_SOURCES] + [os.path.join(emu, "hip_emu_impl.cpp"), os.path.join(emu, "hooks_check.cpp")]
    objs = [str(tmp_path / (os.path.basename(s)[:-4] + ".o")) for s in srcs]

    def compile_one(job):
        src, obj = job
        subprocess.run(base + build.PER_FILE_FLAGS.get(os.path.basename(src), []) + ["-c", src, "-o", obj], check=True)

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        list(ex.map(compile_one, zip(srcs, objs)))
    exe = str(tmp_path / "hooks_check")
    subprocess.run([cxx, "-fsanitize=address,undefined"] + objs + ["-o", exe, "-lpthread"], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-8000:]
    assert "\n0 failures" in p.stdout
