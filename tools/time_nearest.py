"""Cost of vkv_nearest_target (features carried through the envelope passes) next to vkv_distance_transform_weighted with the
same arguments in the SAME run on the SAME buffers: the same passes and the same traffic, g recomputed from the stored feature instead of
loaded.  The cases of tools/time_distance_weighted.py: the bench's C3 volume (1024x1024x795) and the salt-noise scene of
tools/time_filter.py, to the inside at limits 2, 10, 101 and none and to the outside unlimited, weights (1, 1, 1) and (2, 2, 5); the nearest
call with and without d_dist2.  Then vkv_propagate_labels (no mask, and masked by the volume) next to vkv_select_components_by_table, and a
whole Volume.split_bodies next to its parts.  ms from device events (blocks of --calls calls; the variants alternate block by block in one
process, --repeats blocks each after a warm-up call of every variant; median [min .. max]).

    python tools/time_nearest.py [--iso 0.2] [--calls 3] [--repeats 5] [--out profiles/nearest_times.txt]
    python tools/time_nearest.py --rocprof [--out profiles/nearest_rocprof.txt]
                                        per-kernel times under rocprofv3 --kernel-trace --stats (no counters): one child process per scene,
                                        target, limit and call, weights (2, 2, 5), so that no mean mixes cases
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

WEIGHTS = ((1, 1, 1), (2, 2, 5))
CALLS = ("vkv_distance_transform_weighted", "vkv_nearest_target + d_dist2", "vkv_nearest_target")


class Buffers:
    def __init__(self, v):
        self.e, self.vol = v.extent, v.volume
        self.scratch = torch.empty(((lib.distance_transform_scratch_bytes(self.e) + 7) // 8,), dtype=torch.int64, device="cuda")
        self.dist = torch.empty(tuple(self.vol.shape), dtype=torch.int32, device="cuda")
        self.near = torch.empty(tuple(self.vol.shape), dtype=torch.int32, device="cuda")

    def call(self, ctx, name, iso, target, limit, weights):
        args = (self.vol.data_ptr(), self.e, None, iso, dict(TARGETS)[target], weights, limit, self.scratch.data_ptr())
        if name == CALLS[0]:
            ctx.check(ctx.distance_transform_weighted_rc(*args, self.dist.data_ptr(), st()))
        else:
            ctx.check(ctx.nearest_target_rc(*args, self.near.data_ptr(), self.dist.data_ptr() if name == CALLS[1] else None, st()))


def time_volume(ctx, v, iso, calls, repeats, out):
    b = Buffers(v)
    n = b.vol.numel()
    out.append("  volume %dx%dx%d (%.3f G voxels), iso %.3f" % (b.e.width, b.e.height, b.e.depth, n / 1e9, iso))
    for target, limit in CASES:
        for weights in WEIGHTS:
            b.call(ctx, CALLS[0], iso, target, limit, weights)
            want = b.dist.clone()
            b.call(ctx, CALLS[1], iso, target, limit, weights)
            assert torch.equal(want, b.dist), "d_dist2 differs from vkv_distance_transform_weighted"
            found = int((b.near != -1).sum().item())
            del want
            runs = alternate({name: (lambda name=name: b.call(ctx, name, iso, target, limit, weights)) for name in CALLS}, calls, repeats)
            out.append("  to the %s, limit %s, weights %s (%.1f %% of the voxels find a target)" % (target, limit_name(limit), weights, 100.0 * found / n))
            base = statistics.median(runs[CALLS[0]])
            for name in CALLS:
                out.append("    %-32s %s ms  x %5.2f" % (name, fmt(runs[name]), statistics.median(runs[name]) / base))
    return b


def time_propagate_and_split(ctx, v, iso, b, calls, repeats, out):
    """the gather next to the table select (both read one uint32 per voxel and a table / an array through it), and split_bodies whole"""
    labels, _, counts = v.label_components(iso, sizes=False)
    k = int(counts[0].item())
    b.call(ctx, CALLS[2], iso, "inside", None, (1, 1, 1))
    out_labels = torch.empty_like(b.near)
    keep = torch.ones((max(k, 1),), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(b.vol)
    kinds = {
        "vkv_select_components_by_table": lambda: ctx.select_components_by_table(b.vol.data_ptr(), dst.data_ptr(), b.e, None, labels.data_ptr(), keep.data_ptr(), k, 0, st()),
        "vkv_propagate_labels": lambda: ctx.check(ctx.propagate_labels_rc(b.near.data_ptr(), labels.data_ptr(), out_labels.data_ptr(), b.e, None, None, 0.0, st())),
        "vkv_propagate_labels, masked": lambda: ctx.check(ctx.propagate_labels_rc(b.near.data_ptr(), labels.data_ptr(), out_labels.data_ptr(), b.e, None,
                                                                                   b.vol.data_ptr(), iso, st())),
    }
    runs = alternate(kinds, calls, repeats)
    out.append("  the gather (%d components; nearest: to the inside, unlimited)" % k)
    base = statistics.median(runs["vkv_select_components_by_table"])
    for name in kinds:
        out.append("    %-32s %s ms  x %5.2f" % (name, fmt(runs[name]), statistics.median(runs[name]) / base))
    del labels, out_labels, dst
    torch.cuda.empty_cache()
    parts = {
        "Volume.erode(radius2=4)": lambda: v.erode(iso, radius2=4),
        "Volume.label_components": lambda: v.label_components(iso, sizes=False),
        "Volume.nearest_target": lambda: v.nearest_target(iso),
        "Volume.split_bodies(radius2=4)": lambda: v.split_bodies(iso, radius2=4),
    }
    runs = alternate(parts, 1, repeats)
    _, counts = v.split_bodies(iso, radius2=4)
    out.append("  split_bodies (allocations included; %d cores survive the erosion; its label and nearest steps run on the ERODED volume)" % int(counts[0].item()))
    for name in parts:
        out.append("    %-32s %s ms" % (name, fmt(runs[name])))


def measure(ctx, iso, calls, repeats, out):
    out.append("1. c3 (bench.py's volume)")
    v, _, _, _ = bench.build_scene(ctx, "c3")
    b = time_volume(ctx, v, iso, calls, repeats, out)
    time_propagate_and_split(ctx, v, iso, b, calls, repeats, out)
    del v, b
    torch.cuda.empty_cache()
    s, imin = scene_volume(ctx, "salt")
    out.append("2. salt-noise scene (tools/time_filter.py's: shells under hash noise 0..20)")
    V.default_scene(s)
    b = time_volume(ctx, s, imin, calls, repeats, out)
    time_propagate_and_split(ctx, s, imin, b, calls, repeats, out)


def one_case(ctx, scene, iso, target, limit, name, calls):
    """the child of --rocprof: ONE scene, target, limit and call, and nothing else that launches a distance kernel"""
    v, salt_iso = scene_volume(ctx, scene)
    b = Buffers(v)
    for _ in range(calls + 1):
        b.call(ctx, name, salt_iso if scene == "salt" else iso, target, limit, (2, 2, 5))
    torch.cuda.synchronize()


def rocprof(args):
    lines = ["# rocprofv3 --kernel-trace --stats on one MI355X, no counters, ONE child process per scene, target, limit and call (`--only`; %d" % (args.calls + 1),
             "# calls with weights (2, 2, 5) and nothing else): mean ms per dispatch of every distance kernel.  k_env_axis runs twice per call (y, then z):",
             "# its mean is over both passes; k_near_axis<1> is the y pass and k_near_axis<2> the z pass."]
    for scene in ("c3", "salt"):
        for target, limit in CASES:
            for k, name in enumerate(CALLS[:2]):
                only = "%s:%s:%s:%d" % (scene, target, limit_name(limit), k)
                print("profiling " + only, file=sys.stderr, flush=True)
                rows = kernel_stats(__file__, ["--only", only, "--calls", str(args.calls), "--iso", str(args.iso)], 300, quiet=True)
                lines.append("%s, to the %s, limit %s: %s" % (scene, target, limit_name(limit), name))
                total = 0.0
                for r in sorted(rows, key=lambda r: r["Name"]):
                    if "k_edt_" in r["Name"] or "k_env_" in r["Name"] or "k_near_" in r["Name"]:
                        kernel = kernel_name(r["Name"])
                        mean = float(r["AverageNs"]) / 1e6
                        lines.append("    %-16s %4d dispatches %10.4f ms" % (kernel, int(r["Calls"]), mean))
                        total += mean * (2.0 if kernel == "k_env_axis" else 1.0)
                lines.append("    %-16s %15s %10.4f ms" % ("one call", "", total))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iso", type=float, default=0.2, help="the iso of the c3 cases (the salt scene has its own)")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--only", default=None, help="scene:target:limit:call - one case alone, untimed (what --rocprof runs under the profiler)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def only(ctx):
        scene, target, limit, call = args.only.split(":")
        one_case(ctx, scene, args.iso, target, None if limit == "none" else int(limit), CALLS[int(call)], args.calls)

    def plain(ctx):
        lines = ["# tools/time_nearest.py --iso %s --calls %d --repeats %d on one MI355X (device events; median [min .. max]; x: against" % (
            args.iso, args.calls, args.repeats), "# the first call of the same block: the yardstick of the same run)"]
        measure(ctx, args.iso, args.calls, args.repeats, lines)
        return lines

    run(args, plain, lambda: rocprof(args), only, times_name="nearest_times.txt", rocprof_name="nearest_rocprof.txt")


if __name__ == "__main__":
    main()
