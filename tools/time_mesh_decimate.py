"""Cost of decimating an indexed label mesh on the device by vertex clustering (vkv_mesh_decimate) next to its two yardsticks, the extraction that
produced the mesh (vkv_label_mesh_indexed's full call) and one pass of vkv_mesh_smooth over it, in one run on the same buffers.

On the bench's C3 volume (1024x1024x795) with the labels of label_components(iso, 14) and on the salt-noise scene.  Per scene:
  indexed full                   vkv_label_mesh_indexed, vertices, indices and triangle labels: the first yardstick
  one smoothing pass             vkv_mesh_smooth with one factor (the pass and the copy back), its adjacency built beforehand: the second
  decimate, cell c               the whole vkv_mesh_decimate call at c = 2, 4 and 8 voxels per cell, labels and vertex map included
  counting call, cell c          the same with both output capacities zero and no map
with, per cell size, the output's triangles, vertices and bytes against the input's, the scratch block's bytes, and the bytes the call must
touch per second of its time: the input's vertices (12 B) and, twice, its indices (12 B) and the three cells a face gathers (12 B), its labels
for the faces kept, the cell of every vertex written (4 B), 32 B per grid cell cleared and 32 B read back, and everything written.
ms from device events
(blocks of --calls calls; the variants alternate block by block in one process, --repeats blocks each after a warm-up call of every variant;
median [min .. max]).

    python tools/time_mesh_decimate.py [--iso 0.5] [--calls 2] [--repeats 5] [--no-salt] [--out profiles/mesh_decimate_times.txt]
    python tools/time_mesh_decimate.py --rocprof [--out profiles/mesh_decimate_rocprof.txt]   the C3 scene (one block of one call) under rocprofv3
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
from vkvolume_amd import abi, labels as LB, mesh as M  # noqa: E402

CELLS = (2, 4, 8)


def measure(ctx, v, labels, vol, iso, name, calls, repeats, out):
    e = v.extent
    scratch = torch.empty((LB.mesh_indexed_scratch_bytes(e) // 8,), dtype=torch.int64, device="cuda")
    counts = torch.zeros((4,), dtype=torch.int64, device="cuda")

    def extract(vert, idx, tl, nv, nt):
        ctx.check(ctx.label_mesh_indexed_rc(labels.data_ptr(), e, None, None, 0, None if vol is None else vol.data_ptr(), iso, None, None, scratch.data_ptr(),
                                            None if vert is None else vert.data_ptr(), None, None, nv, None if idx is None else idx.data_ptr(),
                                            None if tl is None else tl.data_ptr(), nt, counts.data_ptr(), st()))

    extract(None, None, None, 0, 0)
    nt, _, nv, _ = counts.cpu().tolist()
    vert = torch.empty((max(nv, 1), 3), dtype=torch.float32, device="cuda")
    smoothed, swap = torch.empty_like(vert), torch.empty_like(vert)        # the pass works on a copy: the decimations read the extraction's positions
    idx = torch.empty((max(nt, 1), 3), dtype=torch.int32, device="cuda")
    tl = torch.empty((max(nt, 1),), dtype=torch.int32, device="cuda")
    adjacency = torch.empty((M.adjacency_scratch_bytes(nv, nt) // 8,), dtype=torch.int64, device="cuda")
    in_bytes = 12 * nv + 16 * nt
    out.append("%s: %d triangles, %d vertices; the mesh with its labels %.3f GB" % (name, nt, nv, in_bytes / 1e9))
    extract(vert, idx, tl, nv, nt)
    smoothed.copy_(vert)
    ctx.check(ctx.mesh_adjacency_rc(idx.data_ptr(), nt, nv, counts.data_ptr(), adjacency.data_ptr(), st()))
    # the outputs are sized for the finest grid's result, found by its counting call
    grids = {c: M.cluster_grid(e, c) for c in CELLS}
    d_scratch = torch.empty((max(M.decimate_scratch_bytes(nv, nt, g[2]) for g in grids.values()) // 8,), dtype=torch.int64, device="cuda")
    o_counts = torch.zeros((4,), dtype=torch.int64, device="cuda")

    def decimate(which, c, o_vert=None, o_idx=None, o_tl=None, o_map=None, cap_v=0, cap_t=0):
        origin, cell, n = grids[c]
        which.check(which.mesh_decimate_rc(vert.data_ptr(), idx.data_ptr(), tl.data_ptr(), nv, nt, counts.data_ptr(), origin, cell, abi.Extent3D(*n),
                                           d_scratch.data_ptr(), None if o_vert is None else o_vert.data_ptr(), cap_v, None if o_idx is None else o_idx.data_ptr(),
                                           None if o_tl is None else o_tl.data_ptr(), cap_t, None if o_map is None else o_map.data_ptr(), o_counts.data_ptr(), st()))

    sizes = {}
    for c in CELLS:
        decimate(ctx, c)
        sizes[c] = o_counts.cpu().tolist()
    cap_t, cap_v = max(max(s[0] for s in sizes.values()), 1), max(max(s[2] for s in sizes.values()), 1)
    o_vert = torch.empty((cap_v, 3), dtype=torch.float32, device="cuda")
    o_idx = torch.empty((cap_t, 3), dtype=torch.int32, device="cuda")
    o_tl = torch.empty((cap_t,), dtype=torch.int32, device="cuda")
    o_map = torch.empty((max(nv, 1),), dtype=torch.int32, device="cuda")

    kinds = {
        "indexed full": lambda: extract(vert, idx, tl, nv, nt),
        "one smoothing pass": lambda: ctx.check(ctx.mesh_smooth_rc(smoothed.data_ptr(), swap.data_ptr(), nv, counts.data_ptr(), adjacency.data_ptr(), None, [0.5], st())),
    }
    for c in CELLS:
        kinds["decimate, cell %d" % c] = lambda c=c: decimate(ctx, c, o_vert, o_idx, o_tl, o_map, cap_v, cap_t)
        kinds["counting call, cell %d" % c] = lambda c=c: decimate(ctx, c)
    runs = alternate(kinds, calls, repeats)
    extraction, smoothing = statistics.median(runs["indexed full"]), statistics.median(runs["one smoothing pass"])
    for k in kinds:
        ms = statistics.median(runs[k])
        out.append("  %-38s %s ms  (%5.2f x the extraction's full call, %5.2f x one smoothing pass)" % (k, fmt(runs[k]), ms / extraction, ms / smoothing))
    for c in CELLS:
        t, _, nvo, _ = sizes[c]
        n = grids[c][2]
        cells = n[0] * n[1] * n[2]
        out_bytes = 12 * nvo + 16 * t
        touched = 12 * nv + 2 * (12 + 12) * nt + 4 * t + 4 * nv + 64 * cells + out_bytes + 4 * nv
        ms = statistics.median(runs["decimate, cell %d" % c])
        out.append("  cell %d: %d x %d x %d cells, scratch %.3f GB; out %d triangles (%.1f %%), %d vertices (%.1f %%), %.3f GB (%.1f %%); %.2f GB touched, %.0f GB/s"
                   % (c, n[0], n[1], n[2], M.decimate_scratch_bytes(nv, nt, n) / 1e9, t, 100.0 * t / max(nt, 1), nvo, 100.0 * nvo / max(nv, 1), out_bytes / 1e9,
                      100.0 * out_bytes / max(in_bytes, 1), touched / 1e9, touched / 1e6 / ms))


def rocprof(args):
    rows = kernel_stats(__file__, ["--iso", str(args.iso), "--calls", "1", "--repeats", "1", "--no-salt", "--out", os.devnull], 900)
    return ["# rocprofv3 --kernel-trace --stats of `tools/time_mesh_decimate.py --iso %s --calls 1 --repeats 1 --no-salt` on one MI355X, a run of its own:" % args.iso,
            "# the kernels of vkv_mesh_decimate (k_mdec_*) over the C3 mesh at the cell sizes 2, 4 and 8 (whole calls and counting calls together), next to",
            "# those of vkv_mesh_smooth (k_msmooth_*) and of the extraction (k_lmeshi_*), ms per dispatch"
            ] + stats_table(rows, ("k_mdec_", "k_msmooth_", "k_lmeshi_"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iso", type=float, default=0.5)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-salt", action="store_true")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def plain(ctx):
        lines = ["# tools/time_mesh_decimate.py --iso %s --calls %d --repeats %d on one MI355X (device events; median [min .. max])" % (args.iso, args.calls, args.repeats)]
        v, _, _, _ = bench.build_scene(ctx, "c3")
        labels = v.label_components(args.iso, connectivity=14, sizes=False)[0]
        measure(ctx, v, labels, v.volume, args.iso, "c3, label_components(14), vertices from the volume", args.calls, args.repeats, lines)
        del v, labels
        torch.cuda.empty_cache()
        if not args.no_salt:
            v, iso = scene_volume(ctx, "salt")
            labels = v.label_components(iso, connectivity=14, sizes=False)[0]
            measure(ctx, v, labels, v.volume, iso, "salt, label_components(14), vertices from the volume", args.calls, args.repeats, lines)
        return lines

    run(args, plain, lambda: rocprof(args), times_name="mesh_decimate_times.txt", rocprof_name="mesh_decimate_rocprof.txt")


if __name__ == "__main__":
    main()
