"""The library's pure host arithmetic (vkvolume_amd/host/host_arith.cpp: start orders and the tile mix, the screen bound of the clipped box
and its tile rectangle, the tuning block's defaults, environment and range checks, the opacity table, tile rectangles) as a stand-alone
program under AddressSanitizer + UndefinedBehaviorSanitizer: tests/host_arith_driver.cpp, built from the product's own plain C++ sources
with g++ - no HIP, nothing loaded into Python - and run as a child process.  The driver works its expected values out from the
definitions.  CPU only; a few seconds."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vkvolume_amd", "host")
BUILD = ["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g", "-Wall"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_arithmetic_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "host_arith_driver")
    sources = [os.path.join(ROOT, "tests", "host_arith_driver.cpp"), os.path.join(HOST, "host_arith.cpp"), os.path.join(HOST, "load_volume.cpp")]
    subprocess.check_call(BUILD + sources + ["-o", exe])
    # the driver sets the tuning variables itself: none of the caller's may leak into its "nothing set" case
    env = {k: v for k, v in os.environ.items() if not k.startswith("VKV_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "host arith driver: ok" in r.stdout, r.stdout[-4000:]

