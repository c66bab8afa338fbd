"""Cost of vkv_distance_transform_weighted (lower envelopes, one line per lane) next to vkv_distance_transform in the SAME
run on the SAME buffers: the bench's C3 volume (1024x1024x795) and the salt-noise scene of tools/time_filter.py, to the inside at limits 2,
10, 101 and none and to the outside unlimited; the weighted call with weights (1, 1, 1), which gives the unweighted call's bytes, and (2, 2,
5), the spacing of a 0.5 x 0.5 x 1.25 mm scan (its limits are in weighted units, so the same number is a smaller ball).  ms from device
events (blocks of --calls calls; the three variants alternate block by block in one process, --repeats blocks each after a warm-up call of
every variant; median [min .. max]); GB/s counts the 21 algorithmic bytes per voxel of a transform, as tools/time_distance.py does.

    python tools/time_distance_weighted.py [--iso 0.2] [--calls 3] [--repeats 5] [--out profiles/distance_weighted_times.txt]
    python tools/time_distance_weighted.py --rocprof [--out profiles/distance_weighted_rocprof.txt]
                                        per-kernel times under rocprofv3 --kernel-trace --stats (no counters): one child process per scene,
                                        target, limit and call, so that no mean mixes cases
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.measure import alternate, fmt, kernel_name, kernel_stats, run, stream as st  # noqa: E402
from tools.scenes import CASES, TARGETS, limit_name, scene_volume  # noqa: E402
from vkvolume_amd import lib, volume as V  # noqa: E402

CALLS = (("vkv_distance_transform", None), ("weighted (1, 1, 1)", (1, 1, 1)), ("weighted (2, 2, 5)", (2, 2, 5)))


class Buffers:
    def __init__(self, v):
        self.e, self.vol = v.extent, v.volume
        self.scratch = torch.empty(((lib.distance_transform_scratch_bytes(self.e) + 7) // 8,), dtype=torch.int64, device="cuda")
        self.dist = torch.empty(tuple(self.vol.shape), dtype=torch.int32, device="cuda")

    def transform(self, ctx, iso, target, limit, weights):
        args = (self.vol.data_ptr(), self.e, None, iso, dict(TARGETS)[target])
        if weights is None:
            ctx.distance_transform(*args, limit, self.scratch.data_ptr(), self.dist.data_ptr(), st())
        else:
            ctx.check(ctx.distance_transform_weighted_rc(*args, weights, limit, self.scratch.data_ptr(), self.dist.data_ptr(), st()))


def time_volume(ctx, v, iso, calls, repeats, out):
    b = Buffers(v)
    n = b.vol.numel()
    out.append("  volume %dx%dx%d (%.3f G voxels), iso %.3f" % (b.e.width, b.e.height, b.e.depth, n / 1e9, iso))
    for target, limit in CASES:
        b.transform(ctx, iso, target, limit, None)
        want = b.dist.clone()
        b.transform(ctx, iso, target, limit, (1, 1, 1))
        assert torch.equal(want, b.dist), "weights (1, 1, 1) differ from vkv_distance_transform"
        del want
        runs = alternate({name: (lambda w=w: b.transform(ctx, iso, target, limit, w)) for name, w in CALLS}, calls, repeats)
        out.append("  to the %s, limit %s" % (target, limit_name(limit)))
        base = statistics.median(runs[CALLS[0][0]])
        for name, _ in CALLS:
            m = statistics.median(runs[name])
            out.append("    %-26s %s ms  %7.1f GB/s  x %5.2f" % (name, fmt(runs[name]), 21 * n / 1e9 / (m * 1e-3), m / base))


def measure(ctx, iso, calls, repeats, out):
    out.append("1. c3 (bench.py's volume)")
    v, _, _, _ = bench.build_scene(ctx, "c3")
    time_volume(ctx, v, iso, calls, repeats, out)
    del v
    torch.cuda.empty_cache()
    s, imin = scene_volume(ctx, "salt")
    out.append("2. salt-noise scene (tools/time_filter.py's: shells under hash noise 0..20)")
    V.default_scene(s)
    time_volume(ctx, s, imin, calls, repeats, out)


def one_case(ctx, scene, iso, target, limit, weights, calls):
    """the child of --rocprof: ONE scene, target, limit and call, and nothing else that launches a distance kernel"""
    v, salt_iso = scene_volume(ctx, scene)
    b = Buffers(v)
    for _ in range(calls + 1):
        b.transform(ctx, salt_iso if scene == "salt" else iso, target, limit, weights)
    torch.cuda.synchronize()


def rocprof(args):
    lines = ["# rocprofv3 --kernel-trace --stats on one MI355X, no counters, ONE child process per scene, target, limit and call (`--only`; %d" % (args.calls + 1),
             "# transforms and nothing else): mean ms per dispatch of every distance kernel.  k_edt_axis and k_env_axis run twice per transform (y, then z):",
             "# their mean is over both passes."]
    for scene in ("c3", "salt"):
        for target, limit in CASES:
            for name, weights in CALLS:
                only = "%s:%s:%s:%s" % (scene, target, limit_name(limit), "none" if weights is None else "%d,%d,%d" % weights)
                print("profiling " + only, file=sys.stderr, flush=True)
                rows = kernel_stats(__file__, ["--only", only, "--calls", str(args.calls), "--iso", str(args.iso)], 300, quiet=True)
                lines.append("%s, to the %s, limit %s: %s" % (scene, target, limit_name(limit), name))
                total = 0.0
                for r in sorted(rows, key=lambda r: r["Name"]):
                    if "k_edt_" in r["Name"] or "k_env_" in r["Name"]:
                        kernel = kernel_name(r["Name"])
                        mean = float(r["AverageNs"]) / 1e6
                        lines.append("    %-12s %4d dispatches %10.4f ms" % (kernel, int(r["Calls"]), mean))
                        total += mean * (2.0 if kernel.endswith("_axis") else 1.0)
                lines.append("    %-12s %15s %10.4f ms" % ("one transform", "", total))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iso", type=float, default=0.2, help="the iso of the c3 cases (the salt scene has its own)")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--only", default=None, help="scene:target:limit:weights - one case alone, untimed (what --rocprof runs under the profiler)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def only(ctx):
        scene, target, limit, weights = args.only.split(":")
        one_case(ctx, scene, args.iso, target, None if limit == "none" else int(limit), None if weights == "none" else tuple(int(w) for w in weights.split(",")),
                 args.calls)

    def plain(ctx):
        lines = ["# tools/time_distance_weighted.py --iso %s --calls %d --repeats %d on one MI355X (device events; median [min .. max]; x: against" % (
            args.iso, args.calls, args.repeats), "# vkv_distance_transform of the same block)"]
        measure(ctx, args.iso, args.calls, args.repeats, lines)
        return lines

    run(args, plain, lambda: rocprof(args), only, times_name="distance_weighted_times.txt", rocprof_name="distance_weighted_rocprof.txt")


if __name__ == "__main__":
    main()
