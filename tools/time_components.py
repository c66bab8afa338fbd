"""Cost of connected-component labelling (vkv_label_components) and of the size filter (vkv_select_components) on the bench's C3 volume
and on a salt-noise scene, next to the gradient map and the max map of the same run.

1. C3 (1024x1024x795; bench.py's volume) at each iso, connectivity 6 and 26, dense and through the max map (block 4), all in one run:
     count    the counting call (capacity 0: labels and the three counts, no sizes)
     full     labels + sizes at a capacity of K
     select   vkv_select_components (min_voxels 100) from the full call's results into a second volume
   next to vkv_gradient_map and vkv_max_map of the same volume.  GB/s counts the algorithmic bytes: 1 B read + 4 B written per voxel for the
   labelling, 1 + 4 B read + 1 B written for the selection.
2. The salt-noise scene of tools/time_filter.py (492x492x442, hash noise 0..20 under four thin shells) at the iso of its transfer function's
   lower edge: very many tiny components.
3. One CPU comparison: scipy.ndimage.label on a 256^3 crop of C3 on this host's CPU (one thread), labelled as such.
ms from device events (blocks of --calls calls; the variants alternate block by block in one process, --repeats blocks each after a warm-up
call of every variant; median [min .. max]).

    python tools/time_components.py [--isos 0.2,0.5] [--calls 3] [--repeats 5] [--out profiles/components_times.txt]
    python tools/time_components.py --rocprof [--out profiles/components_rocprof.txt]   per-kernel times under rocprofv3 --kernel-trace --stats:
                                                                 one child process per scene, iso, connectivity and kind of call (count / full),
                                                                 so that no mean mixes scenes or kinds
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
from tools.measure import alternate, fmt, kernel_name, kernel_stats, run, stream as st  # noqa: E402
from tools.scenes import scene_volume  # noqa: E402
from vkvolume_amd import lib, volume as V  # noqa: E402


def time_volume(ctx, v, tf, isos, calls, repeats, out, yardsticks):
    e, me = v.extent, v.map_extent
    n = e.width * e.height * e.depth
    vol = v.volume
    max_map = v.build_max_map()
    scratch = torch.empty((lib.components_scratch_bytes(e) // 8,), dtype=torch.int64, device="cuda")
    counts = torch.zeros((3,), dtype=torch.int64, device="cuda")
    labels = torch.empty(tuple(vol.shape), dtype=torch.int32, device="cuda")
    dst = torch.empty_like(vol)
    out.append("  volume %dx%dx%d (%.3f G voxels), max map %dx%dx%d; scratch %.1f MB, labels %.2f GB" % (
        e.width, e.height, e.depth, n / 1e9, me.width, me.height, me.depth, scratch.numel() * 8 / 1e6, 4 * n / 1e9))

    def label(iso, conn, skip, sizes, cap):
        ctx.label_components(vol.data_ptr(), e, None, iso, conn, max_map.data_ptr() if skip else None, me if skip else None, scratch.data_ptr(),
                             labels.data_ptr(), None if sizes is None else sizes.data_ptr(), cap, counts.data_ptr(), st())

    if yardsticks:
        grad = torch.empty_like(vol)
        runs = alternate({"vkv_gradient_map": lambda: ctx.gradient_map(vol.data_ptr(), grad.data_ptr(), e, tf, st()),
                          "vkv_max_map": lambda: ctx.max_map(vol.data_ptr(), e, me, None, max_map.data_ptr(), st())}, calls, repeats)
        for k, r in runs.items():
            out.append("  %-34s %s ms" % (k, fmt(r)))
        del grad
    for iso in isos:
        for conn in (6, 26):
            label(iso, conn, False, None, 0)
            k, _, inside = counts.cpu().tolist()
            sizes = torch.empty((max(k, 1),), dtype=torch.int32, device="cuda")
            label(iso, conn, False, sizes, k)
            torch.cuda.synchronize()
            largest = int(sizes[:max(k, 1)].max().item()) if k else 0
            out.append("  iso %.3f, connectivity %d: %d components, %d inside voxels (%.2f %%), the largest %d voxels" % (
                iso, conn, k, inside, 100.0 * inside / n, largest))
            kinds = {
                "count, dense": (lambda: label(iso, conn, False, None, 0), 5 * n),
                "count, max map": (lambda: label(iso, conn, True, None, 0), 5 * n),
                "full, dense": (lambda: label(iso, conn, False, sizes, k), 5 * n),
                "full, max map": (lambda: label(iso, conn, True, sizes, k), 5 * n),
            }
            runs = alternate({name: fn for name, (fn, _) in kinds.items()}, calls, repeats)
            # the selection from the last full call's results (the labels are final after every variant: they are the same bytes)
            runs.update(alternate({"select (min_voxels 100)": lambda: ctx.select_components(vol.data_ptr(), dst.data_ptr(), e, None, labels.data_ptr(),
                                                                                            sizes.data_ptr(), counts.data_ptr(), 100, 2 ** 64 - 1, 0, st())},
                                  calls, repeats))
            kinds["select (min_voxels 100)"] = (None, 6 * n)
            for name, (_, nbytes) in kinds.items():
                m = statistics.median(runs[name])
                out.append("    %-32s %s ms  %7.1f GB/s" % (name, fmt(runs[name]), nbytes / 1e9 / (m * 1e-3)))
            assert counts.cpu().tolist() == [k, k, inside]
            del sizes
    return vol


def measure(ctx, isos, calls, repeats, out, cpu):
    out.append("1. c3 (bench.py's volume)")
    v, tf, _, _ = bench.build_scene(ctx, "c3")
    vol = time_volume(ctx, v, tf, isos, calls, repeats, out, True)
    crop = vol[270:526, 384:640, 384:640].cpu().numpy() if cpu else None
    del v, vol
    torch.cuda.empty_cache()
    s, imin = scene_volume(ctx, "salt")
    out.append("2. salt-noise scene (tools/time_filter.py's: shells under hash noise 0..20), iso %.3f" % imin)
    V.default_scene(s)
    time_volume(ctx, s, s.get_transfer_function_uniform(), [imin], calls, repeats, out, False)
    if cpu:
        from scipy import ndimage
        out.append("3. scipy.ndimage.label on a 256^3 crop of c3 (16.8 M voxels) on this host's CPU, one thread; NOT a device time")
        for iso in isos:
            mask = crop.astype("float32") * (1.0 / 255.0) >= iso
            for conn, rank in ((6, 1), (26, 3)):
                t = time.perf_counter()
                _, k = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, rank))
                out.append("  iso %.2f, connectivity %d: %8.1f ms  (%d components)" % (iso, conn, 1e3 * (time.perf_counter() - t), k))


def one_case(ctx, scene, iso, conn, kind, calls):
    """the child of --rocprof: ONE scene, iso, connectivity and kind of call (dense), and nothing else that launches a k_cc_ kernel.  The full
    call takes a capacity of one size per voxel, so that no counting call is needed to size it."""
    v, salt_iso = scene_volume(ctx, scene)
    iso = salt_iso if iso is None else iso
    e, vol = v.extent, v.volume
    n = e.width * e.height * e.depth
    scratch = torch.empty((lib.components_scratch_bytes(e) // 8,), dtype=torch.int64, device="cuda")
    counts = torch.zeros((3,), dtype=torch.int64, device="cuda")
    labels = torch.empty(tuple(vol.shape), dtype=torch.int32, device="cuda")
    sizes = torch.empty((n,), dtype=torch.int32, device="cuda") if kind == "full" else None
    for _ in range(calls + 1):
        ctx.label_components(vol.data_ptr(), e, None, iso, conn, None, None, scratch.data_ptr(), labels.data_ptr(), None if sizes is None else sizes.data_ptr(),
                             n if kind == "full" else 0, counts.data_ptr(), st())
    if kind == "full":
        dst = torch.empty_like(vol)
        for _ in range(calls + 1):
            ctx.select_components(vol.data_ptr(), dst.data_ptr(), e, None, labels.data_ptr(), sizes.data_ptr(), counts.data_ptr(), 100, 2 ** 64 - 1, 0, st())
    torch.cuda.synchronize()
    print("components %d inside %d" % tuple(counts.cpu().tolist()[::2]))


LABEL_KERNELS = ("k_cc_init", "k_cc_merge", "k_cc_flatten", "k_cc_scan_chunks", "k_cc_scan_total", "k_cc_rank_roots", "k_cc_relabel")


def rocprof(args):
    isos = [float(t) for t in args.isos.split(",")]
    cases = [("c3", iso, conn, kind) for iso in isos for conn in (6, 26) for kind in ("count", "full")]
    cases += [("salt", None, conn, kind) for conn in (6, 26) for kind in ("count", "full")]
    lines = ["# rocprofv3 --kernel-trace --stats on one MI355X, ONE child process per scene, iso, connectivity and kind of call (`tools/time_components.py",
             "# --only scene:iso:connectivity:kind --calls %d`: %d dense calls, nothing else): mean ms per dispatch of every kernel of the call, and their" % (
                 args.calls, args.calls + 1),
             "# sum, which is one call's kernel time (the event-timed call of profiles/components_times.txt adds the gaps between its seven launches).",
             "# count = vkv_label_components without sizes; full = with sizes, followed by vkv_select_components (k_cc_select, not part of the sum)."]
    for scene, iso, conn, kind in cases:
        only = "%s:%s:%d:%s" % (scene, "salt" if iso is None else repr(iso), conn, kind)
        keep = {}
        for r in kernel_stats(__file__, ["--only", only, "--calls", str(args.calls)], 300, quiet=True):
            if "k_cc_" in r["Name"]:
                keep[kernel_name(r["Name"])] = (int(r["Calls"]), float(r["AverageNs"]) / 1e6)
        lines.append("%s, iso %s, connectivity %d, %s" % (scene, "0.071" if iso is None else "%.2f" % iso, conn, kind))
        total = 0.0
        for base in LABEL_KERNELS + ("k_cc_select",):
            for name, (ncalls, mean) in keep.items():
                if name.startswith(base):
                    lines.append("    %-24s %4d dispatches %10.4f ms" % (name, ncalls, mean))
                    total += mean if base != "k_cc_select" else 0.0
        lines.append("    %-24s %15s %10.4f ms" % ("sum of one label call", "", total))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--isos", default="0.2,0.5")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--no-cpu", action="store_true", help="leave the scipy comparison out")
    ap.add_argument("--only", default=None, help="scene:iso:connectivity:kind - one case alone, untimed (what --rocprof runs under the profiler)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def only(ctx):
        scene, iso, conn, kind = args.only.split(":")
        one_case(ctx, scene, None if iso == "salt" else float(iso), int(conn), kind, args.calls)

    def plain(ctx):
        lines = ["# tools/time_components.py --isos %s --calls %d --repeats %d on one MI355X (device events; median [min .. max])" % (
            args.isos, args.calls, args.repeats)]
        measure(ctx, [float(t) for t in args.isos.split(",")], args.calls, args.repeats, lines, not args.no_cpu)
        return lines

    run(args, plain, lambda: rocprof(args), only, times_name="components_times.txt", rocprof_name="components_rocprof.txt")


if __name__ == "__main__":
    main()
