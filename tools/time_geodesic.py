"""Cost of vkv_geodesic_propagate (tiles of 8 x 8 x 8 relaxed round by round) next to its yardsticks in the SAME run on the
SAME buffers, on the bench's C3 volume (1024x1024x795) and on the salt-noise scene of tools/time_filter.py:
  1. inside Volume.split_bodies(radius2=4): vkv_nearest_target unlimited + vkv_propagate_labels (the Euclidean hand-back) against the geodesic
     propagation of the same cores' labels through the volume's inside voxels, unlimited, 3-4-5 chamfer, as ONE call of the rounds it needs;
  2. vkv_label_components (26-connected, no sizes) against an unlimited propagation from a single seed, the first inside voxel: the same
     reachability.  That propagation runs as Volume.geodesic_propagate(rounds=None) does, in calls of 64, 128, ... rounds with a host wait
     between them, so its time is wall clock.
Rounds used (found by resumed calls of 1 round in case 1, of 16 in case 2), ms per round, ms per EMPTY round (a resumed call of 64 rounds after the fixed point).
ms from device events (blocks of --calls calls; the variants alternate block by block in one process, --repeats blocks each after a warm-up
call of every variant; median [min .. max]).

    python tools/time_geodesic.py [--iso 0.2] [--calls 2] [--repeats 5] [--scenes c3,salt] [--out profiles/geodesic_times.txt]
    python tools/time_geodesic.py --rocprof [--out profiles/geodesic_rocprof.txt]
                                        per-kernel times under rocprofv3 --kernel-trace --stats (no counters): one child process per scene
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.measure import alternate, event_ms, fmt, kernel_name, kernel_stats, run, stream as st, wall_ms  # noqa: E402
from tools.scenes import scene_volume  # noqa: E402
from vkvolume_amd import abi, geodesic, lib, volume as V  # noqa: E402


class Propagation:
    """the buffers of one vkv_geodesic_propagate over the whole volume of `v`"""

    def __init__(self, ctx, v, iso, seeds):
        self.ctx, self.v, self.iso, self.seeds, self.e = ctx, v, iso, seeds, v.extent
        self.scratch = torch.empty((geodesic.scratch_bytes(self.e) // 8,), dtype=torch.int64, device="cuda")
        self.labels = torch.empty(tuple(v.volume.shape), dtype=torch.int32, device="cuda")
        self.counts = torch.zeros((2,), dtype=torch.int64, device="cuda")

    def call(self, rounds, resume=False):
        self.ctx.check(self.ctx.geodesic_propagate_rc(self.v.volume.data_ptr(), self.e, None, self.iso, None if resume else self.seeds.data_ptr(),
                                                      geodesic.CHAMFER_345, None, rounds, resume, self.scratch.data_ptr(), None, self.labels.data_ptr(),
                                                      self.counts.data_ptr(), st()))

    def rounds_needed(self, step):
        """the rounds after which d_counts[0] is 1, to a multiple of `step` (the round that finds nothing to do included)"""
        self.call(step)
        used = step
        while int(self.counts[0].item()) == 0:
            self.call(step, True)
            used += step
        return used

    def to_the_fixed_point(self):
        """Volume.geodesic_propagate(rounds=None)'s calls: 64, then 128, 256, ... resumed, a host wait between them; the rounds asked for"""
        n = asked = 64
        self.call(n)
        while int(self.counts[0].item()) == 0:
            n = min(2 * n, abi.GEODESIC_MAX_ROUNDS)
            self.call(n, True)
            asked += n
        return asked


def split_case(ctx, v, iso):
    """the eroded volume and its cores' labels, as Volume.split_bodies(radius2=4) makes them"""
    eroded = V.Volume(ctx, v.name + ".eroded", device=v.device)
    eroded.volume, eroded.extent = v.erode(iso, radius2=4), v.extent
    core, _, counts = eroded.label_components(iso, connectivity=6, sizes=False)
    return eroded, core, int(counts[0].item())


def time_scene(ctx, v, iso, calls, repeats, out):
    e = v.extent
    n = e.width * e.height * e.depth
    cc_scratch = torch.empty((lib.components_scratch_bytes(e) // 8,), dtype=torch.int64, device="cuda")
    cc_labels = torch.empty(tuple(v.volume.shape), dtype=torch.int32, device="cuda")
    cc_counts = torch.zeros((3,), dtype=torch.int64, device="cuda")

    def label():
        ctx.label_components(v.volume.data_ptr(), e, None, iso, abi.CONNECT_26, None, None, cc_scratch.data_ptr(), cc_labels.data_ptr(), None, 0, cc_counts.data_ptr(), st())

    label()
    inside = int(cc_counts[2].item())
    first = int(torch.nonzero(cc_labels.view(-1))[0].item())        # the first inside voxel, by the library's own inside rule
    tiles = -(-e.width // 8) * -(-e.height // 8) * -(-e.depth // 8)
    out.append("  volume %dx%dx%d (%.3f G voxels, %.1f %% inside at iso %.3f), %d tiles, state %.2f GB" % (
        e.width, e.height, e.depth, n / 1e9, 100.0 * inside / n, iso, tiles, geodesic.scratch_bytes(e) / 1e9))
    # 1. the hand-back inside split_bodies
    eroded, core, k = split_case(ctx, v, iso)
    p = Propagation(ctx, v, iso, core)
    rounds = p.rounds_needed(1)
    reached = int(p.counts[1].item())
    near_scratch = torch.empty(((lib.distance_transform_scratch_bytes(e) + 7) // 8,), dtype=torch.int64, device="cuda")
    nearest = torch.empty(tuple(v.volume.shape), dtype=torch.int32, device="cuda")
    out_labels = torch.empty(tuple(v.volume.shape), dtype=torch.int32, device="cuda")

    def euclidean():
        ctx.check(ctx.nearest_target_rc(eroded.volume.data_ptr(), e, None, iso, abi.DISTANCE_TO_INSIDE, (1, 1, 1), None, near_scratch.data_ptr(), nearest.data_ptr(),
                                        None, st()))
        ctx.check(ctx.propagate_labels_rc(nearest.data_ptr(), core.data_ptr(), out_labels.data_ptr(), e, None, v.volume.data_ptr(), iso, st()))

    kinds = {"vkv_nearest_target + vkv_propagate_labels": euclidean, "vkv_geodesic_propagate, %d rounds" % rounds: lambda: p.call(rounds)}
    runs = alternate(kinds, calls, repeats)
    euclidean()
    p.call(rounds)
    torch.cuda.synchronize()
    differ = int((out_labels != p.labels).sum().item())
    unlabelled = int(((p.labels == 0) & (out_labels != 0)).sum().item())
    out.append("  1. split_bodies(radius2=4): %d cores; the geodesic call reaches %d voxels in %d rounds (the last finds nothing to do); the two label" % (
        k, reached, rounds))
    out.append("     arrays differ at %d voxels, %d of them labelled by the Euclidean call only" % (differ, unlabelled))
    base = statistics.median(runs["vkv_nearest_target + vkv_propagate_labels"])
    for name in kinds:
        out.append("    %-44s %s ms  x %5.2f" % (name, fmt(runs[name]), statistics.median(runs[name]) / base))
    geo = statistics.median(runs["vkv_geodesic_propagate, %d rounds" % rounds])
    empty = [event_ms(lambda: p.call(64, True), 1) for _ in range(repeats)]        # the state is the fixed point: every workgroup leaves at once
    one = [event_ms(lambda: p.call(1, True), 1) for _ in range(repeats)]           # one empty round and k_geo_finish
    per_empty = (statistics.median(empty) - statistics.median(one)) / 63.0
    out.append("    %-44s %s ms: %.4f ms per empty round; one empty round + k_geo_finish %s ms" % ("64 more rounds at the fixed point", fmt(empty), per_empty, fmt(one)))
    out.append("    %-44s %.3f ms per round (the call less one resumed empty call, over its rounds)" % ("", (geo - statistics.median(one)) / rounds))
    del eroded, core, nearest, out_labels, near_scratch, p
    torch.cuda.empty_cache()
    # 2. reachability: a labelling against a propagation from one seed
    seeds = torch.zeros(tuple(v.volume.shape), dtype=torch.int32, device="cuda")
    seeds.view(-1)[first] = 1
    p = Propagation(ctx, v, iso, seeds)
    rounds = p.rounds_needed(16)
    reached = int(p.counts[1].item())
    label()
    torch.cuda.synchronize()
    body = int((cc_labels == cc_labels.view(-1)[first]).sum().item())
    assert body == reached, (body, reached)
    lab = wall_ms(label, 1, repeats)
    asked = p.to_the_fixed_point()
    geo = wall_ms(p.to_the_fixed_point, 1, max(1, repeats // 2))
    out.append("  2. reachability from the first inside voxel: its body has %d voxels (both calls agree); settled within %d rounds (to 16)" % (body, rounds))
    out.append("    %-44s %s ms (wall clock)" % ("vkv_label_components, 26-connected", fmt(lab)))
    out.append("    %-44s %s ms (wall clock, %d rounds asked for in calls of 64, 128, ...)  x %5.2f" % (
        "vkv_geodesic_propagate to the fixed point", fmt(geo), asked, statistics.median(geo) / statistics.median(lab)))


def scene(ctx, name, iso):
    v, salt_iso = scene_volume(ctx, name)
    if name == "salt":
        V.default_scene(v)
    return v, salt_iso if name == "salt" else iso


def one_case(ctx, name, iso):
    """the child of --rocprof: the geodesic hand-back of split_bodies(radius2=4) on one scene, twice, and nothing else that launches a k_geo_ kernel"""
    v, iso = scene(ctx, name, iso)
    eroded, core, k = split_case(ctx, v, iso)
    p = Propagation(ctx, v, iso, core)
    rounds = p.rounds_needed(1)
    p.call(rounds)
    torch.cuda.synchronize()
    print("ROUNDS %d" % rounds)


def rocprof(args):
    lines = ["# rocprofv3 --kernel-trace --stats on one MI355X, no counters, ONE child process per scene: the geodesic hand-back of",
             "# split_bodies(radius2=4): resumed calls of one round until the state is the fixed point, then one call of that many rounds.",
             "# Mean ms per dispatch; k_geo_round's mean is over full, partial and empty rounds alike."]
    for name in args.scenes.split(","):
        print("profiling " + name, file=sys.stderr, flush=True)
        said = []
        rows = kernel_stats(__file__, ["--only", name, "--iso", str(args.iso)], 600, said=said)
        lines.append("%s (%s)" % (name, ", ".join(x for x in said if x.startswith("ROUNDS"))))
        for r in sorted(rows, key=lambda r: r["Name"]):
            if "k_geo_" in r["Name"]:
                lines.append("    %-16s %5d dispatches %10.4f ms  [%10.4f .. %10.4f]" % (kernel_name(r["Name"]), int(r["Calls"]), float(r["AverageNs"]) / 1e6,
                                                                                 float(r.get("MinNs", "nan")) / 1e6, float(r.get("MaxNs", "nan")) / 1e6))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iso", type=float, default=0.2, help="the iso of the c3 cases (the salt scene has its own)")
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scenes", default="c3,salt")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--only", default=None, help="scene - one case alone, untimed (what --rocprof runs under the profiler)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def plain(ctx):
        lines = ["# tools/time_geodesic.py --iso %s --calls %d --repeats %d on one MI355X (device events unless marked wall clock; median [min .. max];" % (
            args.iso, args.calls, args.repeats), "# x: against the first call of the same block: the yardstick of the same run)"]
        for k, name in enumerate(args.scenes.split(",")):
            lines.append("%d. %s" % (k + 1, {"c3": "c3 (bench.py's volume)", "salt": "salt-noise scene (tools/time_filter.py's: shells under hash noise 0..20)"}[name]))
            v, iso = scene(ctx, name, args.iso)
            time_scene(ctx, v, iso, args.calls, args.repeats, lines)
            del v
            torch.cuda.empty_cache()
        return lines

    run(args, plain, lambda: rocprof(args), lambda ctx: one_case(ctx, args.only, args.iso), times_name="geodesic_times.txt", rocprof_name="geodesic_rocprof.txt")


if __name__ == "__main__":
    main()
