"""Cost of the exact squared Euclidean distance transform (vkv_distance_transform), of the select on it (vkv_select_by_distance) and of a
whole ball opening (Volume.open) on the bench's C3 volume and on a salt-noise scene, next to the gradient map, the 3x3x3 median and the
counting vkv_label_components call of the same run.

1. C3 (1024x1024x795; bench.py's volume) at each iso, both targets, limits 2, 10, 101 and none, all in one run; then the select (1 .. 9 of a
   limit-10 transform) and Volume.open(radius=3), which is two transforms at limit 10 and two selects.  GB/s counts the algorithmic bytes of
   a transform: 1 B read and 4 B written per voxel, and 4 B read + 4 B written for each of the two further passes: 21 B per voxel; the select
   reads 1 + 4 B and writes 1 B.  The work of the y and z passes grows with the distance found, so an unlimited transform is timed by ONE call
   first; when that call takes longer than --slow-ms it is reported as that one call and not repeated.
2. The salt-noise scene of tools/time_filter.py (492x492x442, hash noise 0..20 under four thin shells) at the iso of its transfer function's
   lower edge: targets everywhere, short distances.
3. One CPU comparison, for scale only: scipy.ndimage.distance_transform_edt on a 256^3 crop of C3 on this host's CPU, labelled as such.
ms from device events (blocks of --calls calls; the variants alternate block by block in one process, --repeats blocks each after a warm-up
call of every variant; median [min .. max]).

    python tools/time_distance.py [--isos 0.2,0.5] [--calls 3] [--repeats 5] [--out profiles/distance_times.txt]
    python tools/time_distance.py --rocprof [--limits 10,none] [--out profiles/distance_rocprof.txt]
                                        per-kernel times under rocprofv3 --kernel-trace --stats: one child process per scene, iso, target and
                                        limit, so that no mean mixes cases; with each kernel's algorithmic bytes and the GB/s they make
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.measure import alternate, event_ms, fmt, kernel_name, kernel_stats, run, stream as st  # noqa: E402
from tools.scenes import TARGETS, limit_name, scene_volume  # noqa: E402
from vkvolume_amd import abi, lib, volume as V  # noqa: E402


def time_volume(ctx, v, tf, isos, limits, calls, repeats, slow_ms, out, yardsticks):
    e = v.extent
    n = e.width * e.height * e.depth
    vol = v.volume
    scratch = torch.empty(((lib.distance_transform_scratch_bytes(e) + 7) // 8,), dtype=torch.int64, device="cuda")
    dist = torch.empty(tuple(vol.shape), dtype=torch.int32, device="cuda")
    dst = torch.empty_like(vol)
    out.append("  volume %dx%dx%d (%.3f G voxels); scratch %.2f GB, distances %.2f GB" % (e.width, e.height, e.depth, n / 1e9, scratch.numel() * 8 / 1e9, 4 * n / 1e9))

    def transform(iso, target, limit):
        ctx.distance_transform(vol.data_ptr(), e, None, iso, target, limit, scratch.data_ptr(), dist.data_ptr(), st())

    if yardsticks:
        grad = torch.empty_like(vol)
        cc_scratch = torch.empty((lib.components_scratch_bytes(e) // 8,), dtype=torch.int64, device="cuda")
        counts = torch.zeros((3,), dtype=torch.int64, device="cuda")
        runs = alternate({
            "vkv_gradient_map": lambda: ctx.gradient_map(vol.data_ptr(), grad.data_ptr(), e, tf, st()),
            "vkv_filter_volume median": lambda: ctx.filter_volume(vol.data_ptr(), dst.data_ptr(), e, None, abi.FILTER_MEDIAN3, st()),
            "vkv_label_components count, 6": lambda: ctx.label_components(vol.data_ptr(), e, None, isos[0], 6, None, None, cc_scratch.data_ptr(), dist.data_ptr(),
                                                                          None, 0, counts.data_ptr(), st()),
        }, calls, repeats)
        for k, r in runs.items():
            out.append("  %-34s %s ms" % (k, fmt(r)))
        del grad, cc_scratch
    for iso in isos:
        for tname, target in TARGETS:
            transform(iso, target, 1)
            torch.cuda.synchronize()
            targets = int((dist == 0).sum().item())
            out.append("  iso %.3f, to the %s: %d target voxels (%.2f %%)" % (iso, tname, targets, 100.0 * targets / n))
            kinds = {}
            for limit in limits:
                name = "limit %s" % limit_name(limit)
                if limit is None or limit > 1000:        # one call first: its cost grows with the distances in the volume
                    torch.cuda.synchronize()
                    first = event_ms(lambda: transform(iso, target, limit), 1)
                    if first > slow_ms:
                        far = int(dist.view(torch.uint8).view(torch.int32).to(torch.int64).remainder(1 << 32).max().item())
                        out.append("    %-32s %9.1f ms  %7.1f GB/s  (ONE call, not repeated; the largest value %d)" % (name, first, 21 * n / 1e9 / (first * 1e-3), far))
                        continue
                kinds[name] = lambda limit=limit: transform(iso, target, limit)
            runs = alternate(kinds, calls, repeats)
            for name in kinds:
                m = statistics.median(runs[name])
                out.append("    %-32s %s ms  %7.1f GB/s" % (name, fmt(runs[name]), 21 * n / 1e9 / (m * 1e-3)))
        transform(iso, abi.DISTANCE_TO_OUTSIDE, 10)
        runs = alternate({"select [1, 9] of the last": lambda: ctx.select_by_distance(vol.data_ptr(), dst.data_ptr(), e, None, dist.data_ptr(), 1, 9, 0, st()),
                          "Volume.open(radius=3)": lambda: v.open(iso, radius=3, out=dst)}, calls, repeats)
        for name, nbytes in (("select [1, 9] of the last", 6 * n), ("Volume.open(radius=3)", 2 * (21 + 6) * n)):
            m = statistics.median(runs[name])
            out.append("    %-32s %s ms  %7.1f GB/s" % (name, fmt(runs[name]), nbytes / 1e9 / (m * 1e-3)))
    return vol


def measure(ctx, isos, limits, calls, repeats, slow_ms, out, cpu):
    out.append("1. c3 (bench.py's volume)")
    v, tf, _, _ = bench.build_scene(ctx, "c3")
    vol = time_volume(ctx, v, tf, isos, limits, calls, repeats, slow_ms, out, True)
    crop = vol[270:526, 384:640, 384:640].cpu().numpy() if cpu else None
    del v, vol
    torch.cuda.empty_cache()
    s, imin = scene_volume(ctx, "salt")
    out.append("2. salt-noise scene (tools/time_filter.py's: shells under hash noise 0..20), iso %.3f" % imin)
    V.default_scene(s)
    time_volume(ctx, s, s.get_transfer_function_uniform(), [imin], limits, calls, repeats, slow_ms, out, False)
    if cpu:
        from scipy import ndimage
        out.append("3. scipy.ndimage.distance_transform_edt on a 256^3 crop of c3 (16.8 M voxels) on this host's CPU; NOT a device time")
        for iso in isos:
            mask = crop.astype("float32") * (1.0 / 255.0) >= iso
            for tname, m in (("inside", ~mask), ("outside", mask)):
                t = time.perf_counter()
                ndimage.distance_transform_edt(m)
                out.append("  iso %.2f, to the %s: %8.1f ms" % (iso, tname, 1e3 * (time.perf_counter() - t)))


def one_case(ctx, scene, iso, target, limit, calls):
    """the child of --rocprof: ONE scene, iso, target and limit, then the select, and nothing else that launches a k_edt_ kernel"""
    v, salt_iso = scene_volume(ctx, scene)
    iso = salt_iso if iso is None else iso
    e, vol = v.extent, v.volume
    scratch = torch.empty(((lib.distance_transform_scratch_bytes(e) + 7) // 8,), dtype=torch.int64, device="cuda")
    dist = torch.empty(tuple(vol.shape), dtype=torch.int32, device="cuda")
    dst = torch.empty_like(vol)
    for _ in range(calls + 1):
        ctx.distance_transform(vol.data_ptr(), e, None, iso, dict(TARGETS)[target], limit, scratch.data_ptr(), dist.data_ptr(), st())
        ctx.select_by_distance(vol.data_ptr(), dst.data_ptr(), e, None, dist.data_ptr(), 1, 9, 0, st())
    torch.cuda.synchronize()
    print("voxels %d" % vol.numel())


# kernel: algorithmic bytes per voxel (read + written); k_edt_axis runs twice per call
KERNEL_BYTES = (("k_edt_bits", 1.0 + 1.0 / 8), ("k_edt_x", 1.0 / 8 + 4.0), ("k_edt_axis", 8.0), ("k_edt_select", 6.0))
VOXELS = {"c3": 1024 * 1024 * 795, "salt": 492 * 492 * 442}


def rocprof(args):
    isos = [float(t) for t in args.isos.split(",")]
    limits = [None if t == "none" else int(t) for t in args.limits.split(",")]
    cases = [("c3", iso, t, limit) for iso in isos for t, _ in TARGETS for limit in limits]
    cases += [("salt", None, t, limit) for t, _ in TARGETS for limit in limits]
    lines = ["# rocprofv3 --kernel-trace --stats on one MI355X, ONE child process per scene, iso, target and limit (`tools/time_distance.py --only",
             "# scene:iso:target:limit --calls %d`: %d transforms, each followed by a select, nothing else): mean ms per dispatch of every kernel, the" % (
                 args.calls, args.calls + 1),
             "# algorithmic bytes per voxel of that kernel and the GB/s they make, and the sum over one transform (k_edt_axis twice: the y and the z pass",
             "# are one kernel, so its mean is over both).  Hardware byte counters were not collected."]
    for scene, iso, target, limit in cases:
        only = "%s:%s:%s:%s" % (scene, "salt" if iso is None else repr(iso), target, limit_name(limit))
        print("profiling " + only, file=sys.stderr, flush=True)
        keep = {}
        for r in kernel_stats(__file__, ["--only", only, "--calls", str(args.calls)], 300, quiet=True):
            if "k_edt_" in r["Name"]:
                keep[kernel_name(r["Name"])] = (int(r["Calls"]), float(r["AverageNs"]) / 1e6)
        lines.append("%s, iso %s, to the %s, limit %s" % (scene, "0.071" if iso is None else "%.2f" % iso, target, limit_name(limit)))
        total = 0.0
        for base, per_voxel in KERNEL_BYTES:
            for name, (ncalls, mean) in keep.items():
                if name.startswith(base):
                    lines.append("    %-24s %4d dispatches %10.4f ms  %6.3f B/voxel  %7.1f GB/s" % (name, ncalls, mean, per_voxel,
                                                                                                 per_voxel * VOXELS[scene] / 1e9 / (mean * 1e-3)))
                    total += {"k_edt_axis": 2.0, "k_edt_select": 0.0}.get(base, 1.0) * mean
        lines.append("    %-24s %15s %10.4f ms" % ("sum of one transform", "", total))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--isos", default="0.2,0.5")
    ap.add_argument("--limits", default=None, help="comma-separated, `none` for unlimited (default 2,10,101,none; with --rocprof 10,none)")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slow-ms", type=float, default=500.0, help="an unlimited transform whose first call takes longer is reported as that one call")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--no-cpu", action="store_true", help="leave the scipy comparison out")
    ap.add_argument("--only", default=None, help="scene:iso:target:limit - one case alone, untimed (what --rocprof runs under the profiler)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.limits is None:
        args.limits = "10,none" if args.rocprof else "2,10,101,none"

    def only(ctx):
        scene, iso, target, limit = args.only.split(":")
        one_case(ctx, scene, None if iso == "salt" else float(iso), target, None if limit == "none" else int(limit), args.calls)

    def plain(ctx):
        lines = ["# tools/time_distance.py --isos %s --limits %s --calls %d --repeats %d on one MI355X (device events; median [min .. max])" % (
            args.isos, args.limits, args.calls, args.repeats)]
        measure(ctx, [float(t) for t in args.isos.split(",")], [None if t == "none" else int(t) for t in args.limits.split(",")], args.calls, args.repeats,
                args.slow_ms, lines, not args.no_cpu)
        return lines

    run(args, plain, lambda: rocprof(args), only, times_name="distance_times.txt", rocprof_name="distance_rocprof.txt")


if __name__ == "__main__":
    main()
