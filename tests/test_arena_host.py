"""geo::Arena, the one allocator behind every workspace layout (vqvae_amd/csrc/geo_common.h), as a stand-alone host program
under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/arena_check.hip measures a layout of mixed element sizes,
carves it from a heap block of exactly the measured size, writes every byte, and checks the refusal one byte below and the
optional group both ways.  Nothing is loaded into Python and no device is touched."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_arena_measures_and_carves_under_asan_and_ubsan(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} is missing: the allocator's check needs the compiler the library is built with")
    exe = str(tmp_path / "arena_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host",
           "-fno-omit-frame-pointer"]
    build = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", *san,
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vqvae_amd", "csrc"),
                            os.path.join(ROOT, "tests", "host", "arena_check.hip"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.strip() == "arena_check: ok" and "runtime error" not in run.stderr
