"""Every header of vkvolume_amd/csrc compiles on its own: a translation unit that includes nothing but the header passes the compiler's syntax
check for gfx950 (host and device pass) with the Makefile's FLAGS, so no header depends on what its includer happened to include first.
raymarch_args.hpp, the argument block the host fills, also compiles as plain host C++ with the Makefile's HOSTFLAGS: it holds no device code.
raymarch_inst.hpp is checked without VKV_RAYMARCH_INSTANTIATE, its declarations-only form.  No kernel is instantiated (hipcc needs no GPU;
a few seconds per header; skips without hipcc)."""
import glob
import os
import re
import shutil
import subprocess

import pytest

from tests import helpers as T

HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(T.CSRC, "*.hpp")))


def makefile_flags(variable):
    """the words of `variable` in csrc/Makefile, $(ARCH) = gfx950, other make variables left out (helpers.kernel_listing reads FLAGS the same way)"""
    text = open(os.path.join(T.CSRC, "Makefile")).read().replace("\\\n", " ")
    words = re.search(r"^%s\s*:=\s*(.*)$" % variable, text, flags=re.M).group(1).split()
    return [w.replace("$(ARCH)", "gfx950") for w in words if not w.startswith("$(")]


def syntax_only(header, flags, tmp_path):
    if not os.path.exists(T.HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    unit = tmp_path / "unit.hip"
    unit.write_text('#include "%s"\n' % header)
    cmd = [T.HIPCC if os.path.exists(T.HIPCC) else "hipcc"] + flags + ["-I", T.CSRC, "-fsyntax-only", str(unit)]
    r = subprocess.run(cmd, cwd=T.CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]


def test_the_split_headers_are_there():
    assert {"raymarch_args.hpp", "volume_sampling.hpp", "ray_setup.hpp", "raymarch_persistent.hpp", "raymarch_core.hpp", "raymarch_inst.hpp"} <= set(HEADERS)


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_on_its_own_for_gfx950(header, tmp_path):
    syntax_only(header, makefile_flags("FLAGS"), tmp_path)


def test_raymarch_args_is_plain_host_cxx(tmp_path):
    syntax_only("raymarch_args.hpp", makefile_flags("HOSTFLAGS") + ["-x", "c++"], tmp_path)
