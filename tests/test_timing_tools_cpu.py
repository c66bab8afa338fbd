"""tools/measure.py and tools/scenes.py, which every tools/time_*.py script measures with, as far as they go without a device: reading the
profiler's kernel_stats files, the figures' format, the twenty command lines, the dispatch of a script's main(), and that a failed profiler
child ends the run.  The kernel_stats fixture is a handful of rows of two real rocprofv3 runs on an MI355X (tools/time_mip.py and
tools/time_components.py --only); the help texts are the scripts' own, recorded before they moved onto the shared modules."""
import argparse
import json
import os
import shutil
import stat
import subprocess
import sys

import pytest

from tools import measure, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STATS = os.path.join(GOLDEN, "timing_tools_kernel_stats.csv")
with open(os.path.join(GOLDEN, "timing_tools_help.json")) as _f:
    HELP = json.load(_f)


def test_kernel_names():
    assert measure.kernel_name("void (anonymous namespace)::k_mip<true, false>((anonymous namespace)::MipArgs)") == "k_mip<true, false>"
    assert measure.kernel_name("(anonymous namespace)::k_max_map((anonymous namespace)::MaxMapArgs)") == "k_max_map"
    assert measure.kernel_name("void k_cc_merge<6>(vkv::BoxLinear, unsigned int*, unsigned long const*)") == "k_cc_merge<6>"
    assert measure.kernel_name("k_cc_init(vkv::BoxLinear, vkv::MaxMap, unsigned int*, unsigned long*)") == "k_cc_init"


def test_stripping_the_namespace_changes_nothing_where_it_is_absent():
    """the scripts that did not strip it (one child per case: k_cc_, k_edt_ ...) read the same names as before"""
    plain = [r["Name"] for r in measure.read_kernel_stats(GOLDEN) if "(anonymous namespace)" not in r["Name"]]        # (the fixture's name ends in kernel_stats.csv)
    assert len(plain) == 3
    for name in plain:
        assert measure.kernel_name(name) == (name[5:] if name.startswith("void ") else name).split("(")[0]


def test_read_kernel_stats_one_level_down(tmp_path):
    os.makedirs(tmp_path / "host")
    shutil.copy(STATS, tmp_path / "host" / "1711_kernel_stats.csv")
    (tmp_path / "host" / "1711_kernel_trace.csv").write_text('"Kind"\n"KERNEL_DISPATCH"\n')        # not a stats file
    rows = measure.read_kernel_stats(str(tmp_path))
    got = [(measure.kernel_name(r["Name"]), int(r["Calls"]), int(r["TotalDurationNs"]), float(r["AverageNs"])) for r in rows]
    assert got == [
        ("k_raymarch_lean<0, false, 1, true, 51u>", 4, 8738195, 2184548.75),
        ("k_mip<true, false>", 3, 5750257, 1916752.333333),
        ("k_max_map", 4, 3836377, 959094.25),
        ("k_mip<true, true>", 3, 2965493, 988497.666667),
        ("k_cc_merge<6>", 2, 7615787, 3807893.5),
        ("k_cc_init", 2, 4648577, 2324288.5),
    ]
    assert measure.read_kernel_stats(str(tmp_path / "host")) == rows
    os.makedirs(tmp_path / "empty")
    assert measure.read_kernel_stats(str(tmp_path / "empty")) == []


def test_stats_table():
    rows = measure.read_kernel_stats(GOLDEN)
    assert measure.stats_table(rows, ("k_mip", "k_max_map")) == [
        "%-60s %6s %10s %10s" % ("kernel", "calls", "total ms", "mean ms"),
        "%-60s %6s %10.3f %10.4f" % ("k_mip<true, false>", "3", 5.750257, 1.916752333333),
        "%-60s %6s %10.3f %10.4f" % ("k_max_map", "4", 3.836377, 0.95909425),
        "%-60s %6s %10.3f %10.4f" % ("k_mip<true, true>", "3", 2.965493, 0.988497666667),
    ]


def test_fmt_and_the_distance_cases():
    runs = [1.5, 0.25, 12.125]
    assert measure.fmt(runs) == "%9.4f [%9.4f .. %9.4f]" % (1.5, 0.25, 12.125) == "   1.5000 [   0.2500 ..   12.1250]"
    assert measure.fmt(runs, 7, 3) == "%7.3f [%7.3f .. %7.3f]" % (1.5, 0.25, 12.125) == "  1.500 [  0.250 ..  12.125]"
    assert measure.fmt(runs, width=8) == "%8.4f [%8.4f .. %8.4f]" % (1.5, 0.25, 12.125)
    assert measure.fmt([3.0, 1.0]) == "   2.0000 [   1.0000 ..    3.0000]"
    assert measure.spread([3.0, 1.0, 7.0, 5.0]) == (4.0, 1.0, 7.0)
    assert [scenes.limit_name(x) for x in (None, 2, 101)] == ["none", "2", "101"]
    assert scenes.CASES == (("inside", 2), ("inside", 10), ("inside", 101), ("inside", None), ("outside", None))
    assert [t for t, _ in scenes.TARGETS] == ["inside", "outside"]
    assert scenes.SALT == (4, 200, 0, 0.071)


@pytest.mark.parametrize("script", sorted(HELP))
def test_help_is_unchanged(script):
    """every script starts without a device and answers --help with the text it had before"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", script), "--help"], env=dict(os.environ, COLUMNS="100"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == HELP[script]


def test_the_twenty_scripts():
    assert len(HELP) == 20
    for script in HELP:
        with open(os.path.join(ROOT, "tools", script)) as f:
            text = f.read()
        assert "from tools.time_" not in text and "import tools.time_" not in text, script
        assert '"rocprofv3"' not in text and "torch.cuda.Event(" not in text, script


class Context:
    opened = closed = 0

    def __init__(self):
        Context.opened += 1

    def close(self):
        Context.closed += 1


@pytest.fixture
def root(tmp_path, monkeypatch):
    os.makedirs(tmp_path / "profiles")
    monkeypatch.setattr(measure, "ROOT", str(tmp_path))
    Context.opened = Context.closed = 0
    return tmp_path


def _args(**kw):
    return argparse.Namespace(**dict(dict(out=None, rocprof=False, only=None), **kw))


def _run(args, calls, **kw):
    def plain(ctx):
        calls.append(("plain", type(ctx)))
        return ["# plain", "a 1"]

    def rocprof():
        calls.append(("rocprof", Context.opened))
        return ["# rocprof"]

    def only(ctx):
        calls.append(("only", type(ctx)))

    measure.run(args, plain, rocprof, only, times_name="x_times.txt", rocprof_name="x_rocprof.txt", context=Context, **kw)


def test_run_plain_writes_the_default_and_prints(root, capsys):
    calls = []
    _run(_args(), calls)
    assert calls == [("plain", Context)] and (Context.opened, Context.closed) == (1, 1)
    assert (root / "profiles" / "x_times.txt").read_text() == "# plain\na 1\n"
    assert os.listdir(root / "profiles") == ["x_times.txt"]
    assert capsys.readouterr().out == "# plain\na 1\n"


def test_run_rocprof_opens_no_context(root, capsys):
    calls = []
    _run(_args(rocprof=True), calls)
    assert calls == [("rocprof", 0)] and (Context.opened, Context.closed) == (0, 0)
    assert (root / "profiles" / "x_rocprof.txt").read_text() == "# rocprof\n"
    assert os.listdir(root / "profiles") == ["x_rocprof.txt"]
    assert capsys.readouterr().out == "# rocprof\n"


def test_run_out_wins_over_the_default(root):
    for rocprof, text in ((False, "# plain\na 1\n"), (True, "# rocprof\n")):
        out = root / ("out%d.txt" % rocprof)
        _run(_args(out=str(out), rocprof=rocprof), [])
        assert out.read_text() == text
    assert os.listdir(root / "profiles") == []


def test_run_only_calls_the_case_alone_and_writes_nothing(root, capsys):
    calls = []
    _run(_args(only="c3:1", rocprof=True, out=str(root / "never.txt")), calls)
    assert calls == [("only", Context)] and (Context.opened, Context.closed) == (1, 1)
    assert os.listdir(root / "profiles") == [] and not (root / "never.txt").exists()
    assert capsys.readouterr().out == ""


def test_run_without_a_default_or_echo(root, capsys):
    """time_histogram.py and time_volume_region.py: a file only with --out, and the lines are echoed by the script itself"""
    measure.run(_args(), lambda ctx: ["x"], context=Context, echo=False)
    assert os.listdir(root / "profiles") == [] and capsys.readouterr().out == ""
    measure.run(_args(out=str(root / "o.txt")), lambda ctx: ["x"], context=Context, echo=False)
    assert (root / "o.txt").read_text() == "x\n"


PROFILER = """#!%s
# a stand-in for the profiler: runs the command after `--`; where that succeeds, leaves a kernel_stats file one level below the -d directory
import os, shutil, subprocess, sys
a = sys.argv[1:]
assert a[:4] == ["--kernel-trace", "--stats", "--output-format", "csv"] and a[4] == "-d" and a[6] == "--", a
with open(%r, "a") as f:
    f.write(" ".join(a[7:]) + "\\n")
rc = subprocess.call(a[7:])
if rc == 0:
    os.makedirs(os.path.join(a[5], "host"))
    shutil.copy(%r, os.path.join(a[5], "host", "1_kernel_stats.csv"))
sys.exit(rc)
"""


def test_a_failed_child_stops_the_run(tmp_path, monkeypatch, capfd):
    started = tmp_path / "started.txt"
    exe = tmp_path / "bin" / "rocprofv3"
    os.makedirs(tmp_path / "bin")
    exe.write_text(PROFILER % (sys.executable, str(started), STATS))
    exe.chmod(exe.stat().st_mode | stat.S_IXUSR)
    monkeypatch.setenv("PATH", str(tmp_path / "bin") + os.pathsep + os.environ["PATH"])
    child = tmp_path / "child.py"
    child.write_text("import sys\nprint('ROUNDS 7')\nraise SystemExit(int(sys.argv[1]))\n")
    said = []
    rows = measure.kernel_stats(str(child), ["0"], 60, said=said)
    assert [measure.kernel_name(r["Name"]) for r in rows][1] == "k_mip<true, false>" and said == ["ROUNDS 7"]
    assert len(measure.kernel_stats(str(child), ["0"], 60, quiet=True)) == 6
    assert "ROUNDS" not in capfd.readouterr().out
    done = []
    with pytest.raises(subprocess.CalledProcessError) as e:
        for case in ("0", "3", "0", "0"):        # a caller's plain loop over its cases
            measure.kernel_stats(str(child), [case], 60, quiet=True)
            done.append(case)
    assert e.value.returncode == 3 and done == ["0"]
    assert [line.split()[-1] for line in started.read_text().splitlines()] == ["0", "0", "0", "3"]        # nothing was started after the failure
