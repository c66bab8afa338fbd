"""Cost of measuring labelled components (vkv_component_stats) on the bench's C3 volume and on a salt-noise scene, next to its two
yardsticks from the same run: the pointwise vkv_select_components over the same labels, which reads the same 5 B per voxel, and what the
sizes add to vkv_label_components.

1. C3 (1024x1024x795; bench.py's volume) at each iso, connectivity 6 and 26, all in one run, on the labels of a full label call:
     stats, values      vkv_component_stats with the volume: 4 B of label + 1 B of voxel read per voxel, 80 B written per component
     stats, geometry    the same without the volume (d_volume NULL): 4 B read per voxel
     select (sizes)     vkv_select_components (min_voxels 100) into a second volume: 4 + 1 B read, 1 B written per voxel
     select (table)     vkv_select_components_by_table with the table "at least 100 voxels", computed by torch from the records
     label, count       vkv_label_components without sizes (capacity 0)
     label, full        the same with sizes at a capacity of K; full - count is what the sizes add
   GB/s counts the algorithmic bytes per voxel only.
2. The salt-noise scene of tools/time_filter.py (492x492x442, hash noise 0..20 under four thin shells) at the iso of its transfer function's
   lower edge: millions of tiny components, so the records are hundreds of MB and nearly every entry sends atomics.
ms from device events (blocks of --calls calls; the variants alternate block by block in one process, --repeats blocks each after a warm-up
call of every variant; median [min .. max]).

    python tools/time_component_stats.py [--isos 0.2,0.5] [--calls 3] [--repeats 5] [--out profiles/component_stats_times.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.measure import alternate, fmt, run, stream as st  # noqa: E402
from tools.scenes import scene_volume  # noqa: E402
from vkvolume_amd import abi, lib, volume as V  # noqa: E402


def time_volume(ctx, v, isos, calls, repeats, out):
    e = v.extent
    n = e.width * e.height * e.depth
    vol = v.volume
    scratch = torch.empty((lib.components_scratch_bytes(e) // 8,), dtype=torch.int64, device="cuda")
    counts = torch.zeros((3,), dtype=torch.int64, device="cuda")
    labels = torch.empty(tuple(vol.shape), dtype=torch.int32, device="cuda")
    dst = torch.empty_like(vol)
    out.append("  volume %dx%dx%d (%.3f G voxels); labels %.2f GB" % (e.width, e.height, e.depth, n / 1e9, 4 * n / 1e9))

    def label(iso, conn, sizes, cap):
        ctx.label_components(vol.data_ptr(), e, None, iso, conn, None, None, scratch.data_ptr(), labels.data_ptr(), None if sizes is None else sizes.data_ptr(),
                             cap, counts.data_ptr(), st())

    for iso in isos:
        for conn in (6, 26):
            label(iso, conn, None, 0)
            k, _, inside = counts.cpu().tolist()
            sizes = torch.empty((max(k, 1),), dtype=torch.int32, device="cuda")
            records = torch.empty((max(k, 1), abi.COMPONENT_STATS_BYTES), dtype=torch.uint8, device="cuda")
            label(iso, conn, sizes, k)

            def stats(values):
                ctx.component_stats(vol.data_ptr() if values else None, e, None, labels.data_ptr(), counts.data_ptr(), records.data_ptr(), k, st())

            stats(True)
            torch.cuda.synchronize()
            s = V.ComponentStats(records[:k])
            assert torch.equal(s.voxels, sizes[:k].to(torch.int64)), "the records' voxel counts are not the label call's sizes"
            keep = (s.voxels >= 100).contiguous()
            out.append("  iso %.3f, connectivity %d: %d components (%.1f MB of records), %d inside voxels (%.2f %%), %d components of 100 voxels or more" % (
                iso, conn, k, 80 * k / 1e6, inside, 100.0 * inside / n, int(keep.sum().item())))
            del s
            kinds = {
                "stats, values": (lambda: stats(True), 5 * n),
                "stats, geometry": (lambda: stats(False), 4 * n),
                "select (sizes, min_voxels 100)": (lambda: ctx.select_components(vol.data_ptr(), dst.data_ptr(), e, None, labels.data_ptr(), sizes.data_ptr(),
                                                                                 counts.data_ptr(), 100, 2 ** 64 - 1, 0, st()), 6 * n),
                "select (table, >= 100 voxels)": (lambda: ctx.select_components_by_table(vol.data_ptr(), dst.data_ptr(), e, None, labels.data_ptr(),
                                                                                         keep.data_ptr() if k else None, k, 0, st()), 6 * n),
            }
            runs = alternate({name: fn for name, (fn, _) in kinds.items()}, calls, repeats)
            # the label calls last: they rewrite the labels (to the same bytes) and the sizes
            kinds["label, count"] = (lambda: label(iso, conn, None, 0), 5 * n)
            kinds["label, full"] = (lambda: label(iso, conn, sizes, k), 5 * n)
            runs.update(alternate({name: kinds[name][0] for name in ("label, count", "label, full")}, calls, repeats))
            med = {name: statistics.median(r) for name, r in runs.items()}
            for name, (_, nbytes) in kinds.items():
                out.append("    %-32s %s ms  %7.1f GB/s" % (name, fmt(runs[name]), nbytes / 1e9 / (med[name] * 1e-3)))
            added = med["label, full"] - med["label, count"]
            out.append("    sizes add %.3f ms to the label call; stats, values = %.2f x the select by sizes, %.2f x what the sizes add; stats, geometry = %.2f x "
                       "the select" % (added, med["stats, values"] / med["select (sizes, min_voxels 100)"],
                                       med["stats, values"] / added if added > 0 else float("nan"), med["stats, geometry"] / med["select (sizes, min_voxels 100)"]))
            del sizes, records, keep


def measure(ctx, isos, calls, repeats, out):
    out.append("1. c3 (bench.py's volume)")
    v = bench.build_scene(ctx, "c3")[0]
    time_volume(ctx, v, isos, calls, repeats, out)
    del v
    torch.cuda.empty_cache()
    s, imin = scene_volume(ctx, "salt")
    out.append("2. salt-noise scene (tools/time_filter.py's: shells under hash noise 0..20), iso %.3f" % imin)
    time_volume(ctx, s, [imin], calls, repeats, out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--isos", default="0.2,0.5")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def plain(ctx):
        lines = ["# tools/time_component_stats.py --isos %s --calls %d --repeats %d on one MI355X (device events; median [min .. max])" % (
            args.isos, args.calls, args.repeats)]
        measure(ctx, [float(t) for t in args.isos.split(",")], args.calls, args.repeats, lines)
        return lines

    run(args, plain, times_name="component_stats_times.txt")


if __name__ == "__main__":
    main()
