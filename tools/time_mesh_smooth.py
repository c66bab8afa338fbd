"""Cost of smoothing an indexed label mesh on the device (vkv_mesh_adjacency, vkv_mesh_smooth, vkv_mesh_vertex_normals) next to the extraction
that produced it (vkv_label_mesh_indexed's full call), in one run on the same buffers: is smoothing dearer than extraction?

On the bench's C3 volume (1024x1024x795) with the labels of label_components(iso, 14), on its split_bodies(radius2=4) labels at midpoints
(bodies that touch: the case smoothing is for) and on the salt-noise scene.  Per scene:
  indexed full                   vkv_label_mesh_indexed, vertices, indices and triangle labels: the yardstick
  adjacency build                vkv_mesh_adjacency, once per mesh
  one pass / two passes          vkv_mesh_smooth with one factor (the pass and the copy back into d_vertices) and with two (no copy)
  ten Taubin iterations          twenty passes
  normals, all faces / label 1   vkv_mesh_vertex_normals without and with the label filter
and the adjacency block's bytes next to the mesh's (12 per vertex, 12 per triangle).  ms from device events (blocks of --calls calls; the
variants alternate block by block in one process, --repeats blocks each after a warm-up call of every variant; median [min .. max]).  The
positions drift from block to block (the extraction in the rotation rewrites them); no kernel's work depends on their values.

    python tools/time_mesh_smooth.py [--iso 0.2] [--calls 3] [--repeats 5] [--no-salt] [--out profiles/mesh_smooth_times.txt]
    python tools/time_mesh_smooth.py --rocprof [--out profiles/mesh_smooth_rocprof.txt]   the C3 scenes (one block of one call) under rocprofv3
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
from vkvolume_amd import labels as LB, mesh as M  # noqa: E402

TAUBIN = [0.5, -0.53] * 10


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
    swap, normals = torch.empty_like(vert), torch.empty_like(vert)
    idx = torch.empty((max(nt, 1), 3), dtype=torch.int32, device="cuda")
    tl = torch.empty((max(nt, 1),), dtype=torch.int32, device="cuda")
    nbytes = M.adjacency_scratch_bytes(nv, nt)
    adjacency = torch.empty((nbytes // 8,), dtype=torch.int64, device="cuda")
    out.append("%s: %d triangles, %d vertices; the mesh %.3f GB (12 B per vertex, 12 B per triangle), the adjacency block %.3f GB (%.2f x)" % (
        name, nt, nv, (12 * nv + 12 * nt) / 1e9, nbytes / 1e9, nbytes / max(12 * nv + 12 * nt, 1)))

    def smooth(factors):
        ctx.check(ctx.mesh_smooth_rc(vert.data_ptr(), swap.data_ptr(), nv, counts.data_ptr(), adjacency.data_ptr(), None, factors, st()))

    def vertex_normals(d_labels):
        ctx.check(ctx.mesh_vertex_normals_rc(vert.data_ptr(), idx.data_ptr(), d_labels, 1, nv, nt, counts.data_ptr(), adjacency.data_ptr(), normals.data_ptr(),
                                             st()))

    kinds = {
        "indexed full": lambda: extract(vert, idx, tl, nv, nt),
        "adjacency build": lambda: ctx.check(ctx.mesh_adjacency_rc(idx.data_ptr(), nt, nv, counts.data_ptr(), adjacency.data_ptr(), st())),
        "one pass (and the copy back)": lambda: smooth(TAUBIN[:1]),
        "two passes": lambda: smooth(TAUBIN[:2]),
        "ten Taubin iterations": lambda: smooth(TAUBIN),
        "normals, all faces": lambda: vertex_normals(None),
        "normals, label 1": lambda: vertex_normals(tl.data_ptr()),
    }
    runs = alternate(kinds, calls, repeats)
    base = statistics.median(runs["indexed full"])
    for k in kinds:
        out.append("  %-30s %s ms  (%5.2f x the extraction's full call)" % (k, fmt(runs[k]), statistics.median(runs[k]) / base))
    # the degrees the gathers walk, read out of the block (its layout: mesh_smooth.hip)
    head = adjacency[:4].cpu().tolist()
    chunks = (nv + 4095) // 4096
    degree = adjacency[4 + chunks + 2 * ((nv + 1) // 2):].view(torch.int32)[:nv]
    out.append("  corners of used faces %d; neighbours per vertex: mean %.2f, max %d" % (head[0], float(degree.float().mean()) if nv else 0.0,
                                                                                      int(degree.max()) if nv else 0))


def rocprof(args):
    rows = kernel_stats(__file__, ["--iso", str(args.iso), "--calls", "1", "--repeats", "1", "--no-salt", "--out", os.devnull], 900)
    return ["# rocprofv3 --kernel-trace --stats of `tools/time_mesh_smooth.py --iso %s --calls 1 --repeats 1 --no-salt` on one MI355X, a run of its own:" % args.iso,
            "# the kernels of vkv_mesh_adjacency (k_madj_*), vkv_mesh_smooth (k_msmooth_*), vkv_mesh_vertex_normals (k_mnormals) and of the extraction",
            "# (k_lmeshi_*) over both C3 meshes (the 14-components' and the split bodies'), ms per dispatch"
            ] + stats_table(rows, ("k_madj_", "k_msmooth_", "k_mnormals", "k_lmeshi_"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iso", type=float, default=0.2)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-salt", action="store_true")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def plain(ctx):
        lines = ["# tools/time_mesh_smooth.py --iso %s --calls %d --repeats %d on one MI355X (device events; median [min .. max])" % (args.iso, args.calls, args.repeats)]
        v, _, _, _ = bench.build_scene(ctx, "c3")
        labels = v.label_components(args.iso, connectivity=14, sizes=False)[0]
        measure(ctx, v, labels, v.volume, args.iso, "c3, label_components(14), vertices from the volume", args.calls, args.repeats, lines)
        del labels
        torch.cuda.empty_cache()
        labels, _ = v.split_bodies(args.iso, radius2=4)
        measure(ctx, v, labels, None, 0.0, "c3, split_bodies(radius2=4), midpoints", args.calls, args.repeats, lines)
        del v, labels
        torch.cuda.empty_cache()
        if not args.no_salt:
            v, iso = scene_volume(ctx, "salt")
            labels = v.label_components(iso, connectivity=14, sizes=False)[0]
            measure(ctx, v, labels, v.volume, iso, "salt, label_components(14), vertices from the volume", args.calls, args.repeats, lines)
        return lines

    run(args, plain, lambda: rocprof(args), times_name="mesh_smooth_times.txt", rocprof_name="mesh_smooth_rocprof.txt")


if __name__ == "__main__":
    main()
