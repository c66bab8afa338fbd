"""How the tools/time_*.py scripts measure: the only place that times a call or runs the profiler.

The method, once: one warm-up call of every kind; the kinds alternate block by block in one process; median [min .. max] over the blocks;
a profiler run is a child process of its own with nothing else in it, and the first child that fails or runs out of time ends the run.
A script is its scene, its calls and its report lines; everything else it takes from here and from tools/scenes.py.
"""
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def event_ms(fn, calls):
    """ms per call of one block of `calls` calls, between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(kinds, calls, repeats):
    """{name: [ms per call of each block]}: a warm-up call of every kind, then `repeats` rounds of one block per kind"""
    for fn in kinds.values():
        fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in kinds}
    for _ in range(repeats):
        for k, fn in kinds.items():
            runs[k].append(event_ms(fn, calls))
    return runs


def blocks_ms(fn, warmup, calls, repeats):
    """the one-kind form: `warmup` calls, then `repeats` blocks"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return [event_ms(fn, calls) for _ in range(repeats)]


def wall_ms(fn, calls, repeats, warmup=0):
    """ms per call by the wall clock between two device synchronisations: for calls whose host waits are part of what is measured"""
    for _ in range(warmup):
        fn()
    runs = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) * 1e3 / calls)
    return runs


def spread(runs):
    return statistics.median(runs), min(runs), max(runs)


def fmt(runs, width=9, digits=4):
    """median [min .. max]"""
    one = "%%%d.%df" % (width, digits)
    return (one + " [" + one + " .. " + one + "]") % spread(runs)


def kernel_name(row_name):
    """a kernel_stats row's Name without `void `, the anonymous namespace and the argument list"""
    name = row_name.replace("(anonymous namespace)::", "")
    return (name[5:] if name.startswith("void ") else name).split("(")[0]


def read_kernel_stats(directory):
    """the rows of every *kernel_stats.csv under `directory`, at any depth"""
    rows = []
    for path in sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    return rows


def kernel_stats(script, child_args, timeout, quiet=False, said=None):
    """The kernel_stats rows of `python script child_args` under rocprofv3 --kernel-trace --stats: no counters, no other tracing, one child.
    Raises when the child fails or outlives `timeout` seconds, so a caller's plain loop over its cases starts nothing after that.  `quiet`
    drops the child's output; a list given as `said` receives its lines instead."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(script)] + list(child_args)
        out = subprocess.PIPE if said is not None else subprocess.DEVNULL if quiet else None
        done = subprocess.run(cmd, check=True, timeout=timeout, stdout=out, text=True)
        if said is not None:
            said.extend(done.stdout.splitlines())
        return read_kernel_stats(d)


def stats_table(rows, keep):
    """the per-kernel table of a one-child profile: the rows whose name holds one of `keep`, the largest total first"""
    lines = ["%-60s %6s %10s %10s" % ("kernel", "calls", "total ms", "mean ms")]
    for r in sorted((r for r in rows if any(s in r["Name"] for s in keep)), key=lambda r: -float(r["TotalDurationNs"])):
        lines.append("%-60s %6s %10.3f %10.4f" % (kernel_name(r["Name"])[:60], r["Calls"], float(r["TotalDurationNs"]) / 1e6, float(r["AverageNs"]) / 1e6))
    return lines


def device_context():
    from vkvolume_amd import lib
    torch.cuda.set_device(0)
    return lib.Context(0)


def run(args, plain, rocprof=None, only=None, times_name=None, rocprof_name=None, context=device_context, echo=True):
    """The shape of every main().  With args.only: only(ctx), and no file.  With args.rocprof: the lines of rocprof(), which runs in this
    parent without a context.  Otherwise the lines of plain(ctx).  ctx is a context on device 0, closed afterwards.  The lines go to
    args.out, or to profiles/<times_name> or profiles/<rocprof_name> where there is such a default, and (unless the script has echoed
    them as it went) to stdout."""
    if only is not None and args.only:
        ctx = context()
        only(ctx)
        ctx.close()
        return
    if rocprof is not None and args.rocprof:
        lines, name = rocprof(), rocprof_name
    else:
        ctx = context()
        lines, name = plain(ctx), times_name
        ctx.close()
    text = "\n".join(lines) + "\n"
    path = args.out or (name and os.path.join(ROOT, "profiles", name))
    if path:
        with open(path, "w") as f:
            f.write(text)
    if echo:
        print(text, end="")
