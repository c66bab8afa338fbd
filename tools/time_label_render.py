"""Cost of the label render (vkv_render_labels) and of its visibility map (vkv_label_visibility_map), next to the existing renderer and passes
they stand beside: the shaded isosurface of the same frame at the same iso, vkv_max_map, and vkv_select_components_by_table (the pass a
toggle of one body costs without the label render).

Per scene (c3: bench.py's 1024x1024x795 volume at 1920x1080, labels from label_components(iso 0.2, 26); salt: the salt-noise scene of
tools/time_filter.py at the iso of its transfer function's threshold, where nearly every cell holds a visible voxel), orbit view 0:
  iso dense / maxmap            vkv_render_isosurface, 4 refinement steps: the yardstick
  labels dense / map, shade 0   vkv_render_labels without and with the visibility map, the table's colours as they are
  labels dense / map, shade 1   the same, lit from the volume's gradient at the hit
  every label visible, and every second label hidden (the map is rebuilt for that table)
and the passes: vkv_label_visibility_map, vkv_max_map, vkv_select_components_by_table.  ms per call from device events (blocks of --frames
calls; the kinds alternate block by block in one process, --repeats blocks each, after a warm-up of every kind; median [min .. max]),
samples looked up per covered pixel and hit pixels (d_out_counts).  Every frame writes RGBA8 only.

    python tools/time_label_render.py [--scenes c3,salt] [--frames 10] [--repeats 5] [--out profiles/label_render_times.txt]
    python tools/time_label_render.py --rocprof [--out profiles/label_render_rocprof.txt]   the same run (fewer blocks) under rocprofv3
                                                          --kernel-trace --stats, in a child process of its own, summarised per kernel
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.measure import alternate, fmt, kernel_stats, run, stats_table, stream as st  # noqa: E402
from tools.scenes import scene_volume  # noqa: E402
from vkvolume_amd import abi, labels as LB, volume as V  # noqa: E402

C3_ISO = 0.2


def measure(ctx, name, frames, repeats, out):
    if name == "c3":
        v, _, (w, h), _ = bench.build_scene(ctx, "c3")
        iso = C3_ISO
    else:
        v, iso = scene_volume(ctx, "salt")
        V.default_scene(v)
        V.ComputeGradientMap(ctx).compute(v, v.get_transfer_function_uniform())  # (the packed image that shade == 1 and the isosurface sample)
        w, h = 1920, 1080
    view, proj = bench.cameras(v, w / h)[0]
    v.build_max_map()
    labels, _, counts = v.label_components(iso, connectivity=26, sizes=False)
    k, _, inside = counts.cpu().tolist()
    e, me = v.extent, v.map_extent
    n = e.width * e.height * e.depth
    out.append("%s: volume %dx%dx%d, frame %dx%d, maps %dx%dx%d (block 4); label_components(iso %.3f, 26): %d labels, %d inside voxels (%.2f %%), "
               "labels %.2f GB" % (name, e.width, e.height, e.depth, w, h, me.width, me.height, me.depth, iso, k, inside, 100.0 * inside / n, 4 * n / 1e9))
    sp = V.VolumeRenderSubpass(ctx, v, abi.RenderOptions(skipping_type=abi.SKIP_NONE, early_ray_termination=0), (w, h))
    p = sp.make_params(view, proj)
    rgba8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    counts_px = torch.empty((h, w, 3), dtype=torch.int32, device="cuda")
    tables = {"all visible": torch.from_numpy(LB.color_table(k, seed=1)).cuda(),
              "every second hidden": torch.from_numpy(LB.color_table(k, seed=1, hidden=range(2, k + 1, 2))).cuda()}
    maps = {}
    for tname, table in tables.items():
        maps[tname] = v.build_label_visibility_map(labels, table).clone()
    torch.cuda.synchronize()

    def stats(fn):
        counts_px.zero_()
        rgba8.zero_()
        fn(counts_px)
        torch.cuda.synchronize()
        c = counts_px.view(-1, 3).to(torch.int64)
        covered = int(((c[:, 0] + c[:, 2]) > 0).sum())
        hits = int((rgba8.view(-1, 4)[:, 3] == 255).sum())
        return float(c[:, 0].sum()) / max(1, covered), covered, hits

    def labels_kind(tname, skip, shade):
        def fn(c=None):
            v.label_visibility_map = maps[tname]
            sp.draw_labels(p, labels, tables[tname], shade=shade, rgba8=rgba8, counts=c, skip=skip)
        return fn

    kinds = {}
    for skip in (False, True):
        kinds["iso %.3f %-6s" % (iso, "maxmap" if skip else "dense")] = lambda c=None, skip=skip: sp.draw_iso(p, iso, rgba8=rgba8, counts=c, skip=skip)
    for tname in tables:
        for shade in (False, True):
            for skip in (False, True):
                kinds["labels %-5s shade %d, %s" % ("map" if skip else "dense", shade, tname)] = labels_kind(tname, skip, shade)
    runs = alternate(kinds, frames, repeats)
    base = {skip: statistics.median(runs["iso %.3f %-6s" % (iso, "maxmap" if skip else "dense")]) for skip in (False, True)}
    for kname, fn in kinds.items():
        spp, covered, hits = stats(fn)
        against = base[" map " in kname or "maxmap" in kname]
        out.append("  %-46s %s ms/frame  %5.2fx iso  %8.1f samples per covered pixel (%d covered, %d hit)" % (
            kname, fmt(runs[kname]), statistics.median(runs[kname]) / against, spp, covered, hits))
    # the passes: the map build against the max map and against the selection it replaces when a body is toggled
    keep = torch.ones((max(k, 1),), dtype=torch.uint8, device="cuda")
    keep[1::2] = 0
    dst = torch.empty_like(v.volume)
    vis = torch.empty_like(maps["all visible"])
    passes = {"vkv_max_map": lambda: ctx.max_map(v.volume.data_ptr(), e, me, None, v.max_map.data_ptr(), st()),
              "vkv_select_components_by_table": lambda: ctx.select_components_by_table(v.volume.data_ptr(), dst.data_ptr(), e, None, labels.data_ptr(),
                                                                                        keep.data_ptr(), k, 0, st())}
    for tname, table in tables.items():
        passes["vkv_label_visibility_map, %s" % tname] = lambda table=table: ctx.check(ctx.label_visibility_map_rc(
            labels.data_ptr(), e, None, table.data_ptr() if k else None, k, me, vis.data_ptr(), st()))
    runs = alternate(passes, frames, repeats)
    for kname in passes:
        m = statistics.median(runs[kname])
        nbytes = {"vkv_max_map": n, "vkv_select_components_by_table": 6 * n}.get(kname, 4 * n)
        out.append("  %-46s %s ms/call   %7.1f GB/s of %.2f GB" % (kname, fmt(runs[kname]), nbytes / 1e9 / (m * 1e-3), nbytes / 1e9))
    del v, labels, dst
    torch.cuda.empty_cache()


def rocprof(args):
    rows = kernel_stats(__file__, ["--scenes", args.scenes, "--frames", "3", "--repeats", "1", "--out", os.devnull], 360)
    return ["# rocprofv3 --kernel-trace --stats of `tools/time_label_render.py --scenes %s --frames 3 --repeats 1` on one MI355X, a run of its own:" % args.scenes,
            "# the label render's kernels (k_labels<SHADE, SKIP>: SHADE 0 flat, 1 lit from the linear volume, 2 lit from the packed image; SKIP =",
            "# visibility map), the isosurface kernels of the same frames, and the map and selection passes; ms per dispatch over both scenes"
            ] + stats_table(rows, ("k_labels", "k_label_visibility_map", "k_iso", "k_max_map", "select"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="c3,salt")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def plain(ctx):
        lines = ["# tools/time_label_render.py --scenes %s --frames %d --repeats %d on one MI355X (device events; median [min .. max]);"
                 % (args.scenes, args.frames, args.repeats),
                 "# 'x iso': against vkv_render_isosurface of the same frame and iso in the same run, dense against dense and map against max map"]
        for name in args.scenes.split(","):
            measure(ctx, name, args.frames, args.repeats, lines)
            print("\n".join(lines), flush=True)
        return lines

    run(args, plain, lambda: rocprof(args), times_name="label_render_times.txt", rocprof_name="label_render_rocprof.txt")


if __name__ == "__main__":
    main()
