"""The launch-uniform arithmetic the ray-march kernels take from the host instead of working it out in every wave
(vkvolume_amd/host/host_arith.hpp): UniformDiv, the multiply-and-shift division by a launch's divisors, and the float helpers behind
RayMarchArgs.cells_per_unit and free_margin.  tests/uniform_div_driver.cpp includes the header - the functions are the ones the kernels
compile - and checks, as a stand-alone program under UndefinedBehaviorSanitizer:
  * quotient and remainder against / and % for every divisor 1 ... 65536 (and every power of two with its neighbours up to 2^30) with the
    numerators 0, 1, d - 1, d, d + 1, k d - 1, k d, k d + 1 for hashed k, 2^30 - 1 and the largest numerator the launch checks admit;
  * every numerator below 2^20 for the divisors up to 64;
  * cells_per_unit and the margin against the plain float expressions for extents 1 ... 2048 and block sizes 1 ... 17: an identity today, and
    a guard against a later "optimisation" of the host helpers (the kernels' frames are pinned to the bit by them).
CPU only; a few seconds."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wall"]


def test_uniform_division_and_float_helpers_match_the_plain_expressions(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "uniform_div_driver")
    subprocess.check_call(BUILD + [os.path.join(ROOT, "tests", "uniform_div_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "uniform div driver: ok" in r.stdout, r.stdout[-4000:]
