"""GPU: vkv_mesh_decimate bit for bit against the numpy statement of tests/mesh_decimate_ref.py, in every output: vertices,
faces, face labels, the vertex map and the four counts, and in the bytes past the counts, which must keep their fill.

The meshes: the hand-made ones of tests/mesh_smooth_ref.py; isosurface and label meshes straight from the device extractors on volumes of at
most 40^3 at the cell sizes 2, 3 and (2, 3, 5); a grid of one cell; a grid of 17 x 16 x 16 cells (the cell scan crosses a chunk of 4096) and a
mesh of more than 4096 x 3 faces (the face scan does); fans with more than 64 and more than 4096 vertices in one cell, and runs of equal cells
that straddle lanes 63 | 64 and a workgroup's last thread; short output capacities; a truncated input; labels and the vertex map present and
absent; the output fed to the adjacency, the normals and a second decimation; two runs; a captured graph; every rejection.

Every buffer is a tests/helpers.py guarded() allocation, pre-filled and compared as a whole, so nothing here relies on, or can cause, a fault."""
import numpy as np
import pytest
import torch

from tests import helpers as T
from tests import mesh_decimate_ref as D
from tests import mesh_smooth_ref as R
from vkvolume_amd import abi, labels as LB, lib, mesh as M

pytestmark = pytest.mark.gpu
FILL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    c = lib.Context(0)
    yield c
    c.close()


def st():
    return torch.cuda.current_stream().cuda_stream


def same_u32(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a.view(np.uint32).reshape(-1) != b.view(np.uint32).reshape(-1))
    assert len(bad) == 0, "%s: %d of %d words differ, first at %d: %r != %r" % (what, len(bad), a.size, bad[0], a.reshape(-1)[bad[0]], b.reshape(-1)[bad[0]])


def prefilled(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def expected(want, nv_in, cv_in, out_cv, out_ct, with_labels, with_map):
    """the whole of every output buffer: the statement's prefix, the fill behind it"""
    v, t = len(want["vertices"]), len(want["faces"])
    out = {"counts": np.array([t, min(t, out_ct), v, min(v, out_cv)], np.int64)}
    out["vertices"] = prefilled((max(out_cv, 1), 3), np.float32)
    out["vertices"][:min(v, out_cv)] = want["vertices"][:out_cv]
    out["faces"] = prefilled((max(out_ct, 1), 3), np.uint32)
    out["faces"][:min(t, out_ct)] = want["faces"][:out_ct].astype(np.uint32)
    out["labels"] = prefilled((max(out_ct, 1),), np.uint32)
    if with_labels:
        out["labels"][:min(t, out_ct)] = want["labels"][:out_ct]
    out["map"] = prefilled((max(cv_in, 1),), np.uint32)
    if with_map:
        out["map"][:nv_in] = want["vertex_map"]
    return out


class Run:
    """one vkv_mesh_decimate call on guarded buffers; .got holds every output buffer as a whole"""

    def __init__(self, ctx, vertices, faces, grid, counts=None, face_labels=None, out_cv=None, out_ct=None, with_map=True, what="", want=None):
        self.what = what
        origin, cell, n = D.grid_of(*grid)
        vertices, faces = np.array(vertices, np.float32), np.ascontiguousarray(faces).astype(np.int64)
        cv, ct = len(vertices), len(faces)
        self.h_counts = [ct, ct, cv, cv] if counts is None else [int(c) for c in counts]
        out_cv, out_ct = cv if out_cv is None else out_cv, ct if out_ct is None else out_ct
        self.handles = []
        d_vert = self.buffer("d_vertices", vertices if cv else (1, 3), np.float32)
        d_idx = self.buffer("d_indices", faces.astype(np.uint32).view(np.int32) if ct else (1, 3), np.int32)
        d_tl = None if face_labels is None else self.buffer("d_triangle_labels", np.array(face_labels, np.uint32).view(np.int32) if ct else (1,), np.int32)
        d_counts = self.buffer("d_counts", np.array(self.h_counts, np.int64), np.int64)
        nbytes = M.decimate_scratch_bytes(cv, ct, n)
        assert nbytes == lib.load().vkv_mesh_decimate_scratch_bytes(cv, ct, abi.Extent3D(*n)) and nbytes % 8 == 0 and nbytes > 0
        d_scratch = self.buffer("d_scratch", (nbytes // 8,), np.int64)
        self.out = {
            "vertices": self.buffer("d_out_vertices", (max(out_cv, 1), 3), np.float32),
            "faces": self.buffer("d_out_indices", (max(out_ct, 1), 3), np.int32),
            "labels": self.buffer("d_out_triangle_labels", (max(out_ct, 1),), np.int32),
            "map": self.buffer("d_vertex_map", (max(cv, 1),), np.int32),
            "counts": self.buffer("d_out_counts", (4,), np.int64),
        }
        inputs = [(d, d.cpu().numpy().tobytes()) for d in (d_vert, d_idx, d_counts) + (() if d_tl is None else (d_tl,))]
        ctx.check(ctx.mesh_decimate_rc(d_vert.data_ptr(), d_idx.data_ptr(), None if d_tl is None else d_tl.data_ptr(), cv, ct, d_counts.data_ptr(), origin, cell,
                                       abi.Extent3D(*n), d_scratch.data_ptr(), self.out["vertices"].data_ptr(), out_cv, self.out["faces"].data_ptr(),
                                       self.out["labels"].data_ptr(), out_ct, self.out["map"].data_ptr() if with_map else None, self.out["counts"].data_ptr(), st()))
        torch.cuda.synchronize()
        for name, h in self.handles:
            assert not h.check(), "%s: %s: guard bytes changed" % (what, name)
        for d, before in inputs:
            assert d.cpu().numpy().tobytes() == before, "%s: an input changed" % what
        self.got = {k: v.cpu().numpy() for k, v in self.out.items()}
        for k in ("faces", "labels", "map"):
            self.got[k] = self.got[k].view(np.uint32)
        # `want`: the statement's answer for exactly this mesh and grid, where a caller has it already
        self.want = D.decimate_np(vertices, faces, origin, cell, n, counts=self.h_counts, face_labels=face_labels) if want is None else want
        self.nv = R.bounds(cv, ct, self.h_counts)[0]
        self.expect = expected(self.want, self.nv, cv, out_cv, out_ct, face_labels is not None, with_map)

    def buffer(self, name, array_or_shape, dtype):
        view, handle = T.guarded(array_or_shape, 0, FILL, "cuda", dtype=dtype)
        self.handles.append((name, handle))
        return view

    def check(self):
        assert self.got["counts"].tolist() == self.expect["counts"].tolist(), (self.what, self.got["counts"].tolist(), self.expect["counts"].tolist())
        for k in ("vertices", "faces", "labels", "map"):
            same_u32(self.got[k], self.expect[k], "%s: %s" % (self.what, k))
        return self


def check_variants(ctx, vertices, faces, grid, face_labels, what, counts=None):
    """the full call; labels and the map absent; each output capacity short alone, both, and the counting call: exact totals, exact prefixes"""
    full = Run(ctx, vertices, faces, grid, counts=counts, face_labels=face_labels, what=what).check()
    v, t = len(full.want["vertices"]), len(full.want["faces"])
    Run(ctx, vertices, faces, grid, counts=counts, face_labels=None, with_map=False, what=what + ", no labels, no map").check()
    for out_cv, out_ct in ((v // 2, None), (None, t // 3), (max(v - 1, 0), max(t - 1, 0)), (0, 0), (v, t)):
        Run(ctx, vertices, faces, grid, counts=counts, face_labels=face_labels, out_cv=out_cv, out_ct=out_ct, what="%s, capacities %s %s" % (what, out_cv, out_ct)).check()
    return full


# ---- the hand-made meshes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.small_meshes()))
def test_small_meshes(ctx, name):
    vertices, faces = R.small_meshes()[name]
    labels = (1 + np.arange(len(faces)) % 2).astype(np.uint32)
    for cell in (0.5, 1.0, (0.5, 1.0, 3.0)):
        check_variants(ctx, vertices, faces, D.grid_for(vertices, cell), labels, "%s, cell %s" % (name, cell))


def test_a_grid_of_one_cell(ctx):
    vertices, _, faces, face_labels, _ = R.extracted("junction")
    run = Run(ctx, vertices, faces, ((-0.25,) * 3, 100.0, (1, 1, 1)), face_labels=face_labels, what="one cell").check()
    assert run.got["counts"].tolist() == [0, 0, 0, 0] and (run.got["map"] == D.NONE).all()
    # and with every vertex outside the grid, NaN included: everything is clamped into the one cell
    far = np.array(vertices) + np.float32(1e6)
    far[::7] = np.nan
    Run(ctx, far, faces, ((0,) * 3, 1.0, (1, 1, 1)), what="one cell, far away").check()


def test_positions_outside_the_grid_and_nan_are_clamped(ctx):
    vertices, _, faces, face_labels, _ = R.extracted("junction")
    moved = np.array(vertices)
    moved[::11, 0] = np.nan
    moved[5::13, 1] = -np.inf
    moved[3::17, 2] = 1e30
    run = Run(ctx, moved, faces, ((3.75,) * 3, 2.0, (3, 2, 3)), face_labels=face_labels, with_map=True, what="a grid smaller than the mesh")
    # the means of cells that hold a non-finite position are unspecified; everything else is pinned
    assert run.got["counts"].tolist() == run.expect["counts"].tolist()
    same_u32(run.got["faces"], run.expect["faces"], "faces")
    same_u32(run.got["map"], run.expect["map"], "map")
    wild = ~(np.abs(moved) <= 2.0 ** 20).all(axis=1)        # NaN compares false
    tame = np.ones(len(run.expect["vertices"]), bool)
    tame[np.setdiff1d(run.want["vertex_map"][wild], [D.NONE])] = False
    assert wild.sum() > 100 and tame[:len(run.want["vertices"])].sum() > 3
    same_u32(run.got["vertices"][tame], run.expect["vertices"][tame], "the means of the cells without such a position")


# ---- the scans --------------------------------------------------------------------------------------------------------------------------------
def test_the_cell_scan_crosses_a_chunk(ctx):
    vertices, faces, face_labels = D.ball()
    assert 17 * 16 * 16 > 4096
    run = check_variants(ctx, vertices, faces, ((-0.25,) * 3, 1.25, (17, 16, 16)), face_labels, "17 x 16 x 16 cells")
    named = np.flatnonzero(np.bincount(D.cells_np(vertices, (-0.25,) * 3, 1.25, (17, 16, 16))[faces[run.want["kept"]]].reshape(-1), minlength=17 * 256))
    assert named.min() < 4096 < named.max()        # cells on both sides of the chunk boundary are numbered


def test_faces_in_many_workgroups(ctx):
    vertices, _, faces, face_labels, _ = R.extracted("split ball")
    assert len(faces) > 3 * 4096
    run = check_variants(ctx, vertices, faces, M.cluster_grid((24, 24, 24), 1.0), face_labels, "split ball, cell 1")
    assert run.want["kept"].max() > 2 * 4096 and len(run.want["faces"]) >= 4096


def test_the_face_scan_crosses_a_chunk(ctx):
    """The faces are counted per workgroup of 256 and those counts scanned in chunks of 4096: more than 4096 x 256 faces cross a chunk.  They
    name few vertices, so the statement stays quick"""
    nv, per = 70000, 16
    rng = np.random.default_rng(11)
    vertices = (rng.random((nv, 3), np.float32) * np.float32(19.0)).astype(np.float32)
    i = np.arange(nv - per - 2)
    faces = np.concatenate([np.stack([i, i + 1, i + 2 + k], axis=1) for k in range(per)])
    assert len(faces) > 4096 * 256 + 4096
    labels = (faces[:, 2] % 5).astype(np.uint32)
    grid = ((-0.25,) * 3, 2.0, (10, 10, 10))
    run = Run(ctx, vertices, faces, grid, face_labels=labels, what="a million faces").check()
    kept = run.want["kept"]
    assert (kept < 4096 * 256).sum() > 1000 and (kept >= 4096 * 256).sum() > 1000 and len(kept) < len(faces)
    Run(ctx, vertices, faces, grid, face_labels=labels, out_cv=500, out_ct=len(kept) - 2000, with_map=False, what="a million faces, short", want=run.want).check()


@pytest.mark.parametrize("n", [100, 5000])
def test_fans_with_many_vertices_in_one_cell(ctx, n):
    vertices, faces = D.fan(n, 0.9)
    # one cell for the whole rim (more than 64, more than 4096 vertices in it) and one for the hub: every face collapses, the sums are exact
    run = Run(ctx, vertices, faces, ((0.5,) * 3, 4.0, (3, 3, 3)), what="fan of %d, rim in one cell" % n).check()
    assert run.got["counts"].tolist() == [0, 0, 0, 0]
    # small cells: runs of equal cells of every length along the rim; the faces between two runs and the hub survive
    run = check_variants(ctx, vertices, faces, ((0.5,) * 3, 0.05 if n == 100 else 0.02, (50, 50, 50)), None, "fan of %d, small cells" % n)
    assert 0 < len(run.want["faces"]) < n
    # the hub in the rim's cell as well
    run = Run(ctx, vertices, faces, ((0.5,) * 3, 100.0, (2, 1, 1)), what="fan of %d, everything in one cell of two" % n).check()
    assert run.got["counts"].tolist() == [0, 0, 0, 0]


def test_runs_that_straddle_a_wave_and_a_workgroup(ctx):
    """vertices whose cells change exactly at, one before and one after lanes 63 | 64 and threads 255 | 256, in a strip of triangles"""
    for first in (1, 62, 63, 64, 65, 254, 255, 256, 257, 300):
        n = 700
        x = np.where(np.arange(n) < first, 0.25, 1.25 + (np.arange(n) - first) // 64)        # a run of `first`, then runs of 64
        vertices = np.stack([x, (np.arange(n) % 5) * 0.17, (np.arange(n) % 3) * 0.29], axis=1).astype(np.float32)
        faces = np.stack([np.arange(n - 130), np.arange(n - 130) + 65, np.arange(n - 130) + 130], axis=1)
        run = Run(ctx, vertices, faces, ((0, 0, 0), 1.0, (16, 1, 1)), what="first run of %d" % first).check()
        assert len(run.want["faces"]) > 0


# ---- the extractors' meshes -------------------------------------------------------------------------------------------------------------------
def device_label_mesh(ctx, labels):
    d, h, w = labels.shape
    e = abi.Extent3D(w, h, d)
    d_lab = torch.from_numpy(labels.view(np.int32)).cuda()
    scratch = torch.empty((LB.mesh_indexed_scratch_bytes(e) // 8,), dtype=torch.int64, device="cuda")
    counts = torch.zeros((4,), dtype=torch.int64, device="cuda")
    ctx.check(ctx.label_mesh_indexed_rc(d_lab.data_ptr(), e, None, None, 0, None, 0.0, None, None, scratch.data_ptr(), None, None, None, 0, None, None, 0,
                                        counts.data_ptr(), st()))
    nt, _, nv, _ = counts.cpu().tolist()
    vert = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    idx = torch.empty((nt, 3), dtype=torch.int32, device="cuda")
    tl = torch.empty((nt,), dtype=torch.int32, device="cuda")
    ctx.check(ctx.label_mesh_indexed_rc(d_lab.data_ptr(), e, None, None, 0, None, 0.0, None, None, scratch.data_ptr(), vert.data_ptr(), None, None, nv,
                                        idx.data_ptr(), tl.data_ptr(), nt, counts.data_ptr(), st()))
    torch.cuda.synchronize()
    return vert.cpu().numpy(), idx.cpu().numpy().view(np.uint32).astype(np.int64), tl.cpu().numpy().view(np.uint32), (w, h, d)


def device_iso_mesh(ctx, volume, iso):
    d, h, w = volume.shape
    e = abi.Extent3D(w, h, d)
    d_vol = torch.from_numpy(volume).cuda()
    scratch = torch.empty((lib.mesh_indexed_scratch_bytes(e) // 8,), dtype=torch.int64, device="cuda")
    counts = torch.zeros((4,), dtype=torch.int64, device="cuda")
    ctx.check(ctx.isosurface_mesh_indexed_rc(d_vol.data_ptr(), e, None, iso, None, None, scratch.data_ptr(), None, None, 0, None, 0, counts.data_ptr(), st()))
    nt, _, nv, _ = counts.cpu().tolist()
    vert = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    idx = torch.empty((nt, 3), dtype=torch.int32, device="cuda")
    ctx.check(ctx.isosurface_mesh_indexed_rc(d_vol.data_ptr(), e, None, iso, None, None, scratch.data_ptr(), vert.data_ptr(), None, nv, idx.data_ptr(), nt,
                                             counts.data_ptr(), st()))
    torch.cuda.synchronize()
    return vert.cpu().numpy(), idx.cpu().numpy().view(np.uint32).astype(np.int64), (w, h, d)


@pytest.fixture(scope="module")
def extracted_on_the_device(ctx):
    z, y, x = np.indices((30, 40, 36)).astype(np.float64)
    r = np.sqrt((x - 17.3) ** 2 + (y - 19.1) ** 2 + ((z - 14.6) * 1.2) ** 2)
    volume = np.clip(255.0 * (1.0 - r / 22.0) + 9.0 * np.sin(x * 0.9) * np.cos(y * 0.7), 0, 255).astype(np.uint8)
    iso = device_iso_mesh(ctx, volume, 0.45)
    assert 2000 < len(iso[0]) and len(iso[1]) > 4096
    return {"iso": iso + (None,), "split ball": device_label_mesh(ctx, R.split_ball_labels()), "junction": device_label_mesh(ctx, R.junction_labels())}


@pytest.mark.parametrize("cell", D.CELLS, ids=str)
@pytest.mark.parametrize("name", ["iso", "split ball", "junction"])
def test_meshes_straight_from_the_device_extractors(ctx, extracted_on_the_device, name, cell):
    mesh = extracted_on_the_device[name]
    if name == "iso":
        vertices, faces, extent, labels = mesh
    else:
        vertices, faces, labels, extent = mesh
    run = Run(ctx, vertices, faces, M.cluster_grid(extent, cell), face_labels=labels, what="%s, cell %s" % (name, cell)).check()
    assert 0 < len(run.want["faces"]) < len(faces) and 0 < len(run.want["vertices"]) < len(vertices)
    if name != "iso":        # closedness, exactly, on the device's bytes
        t = run.got["counts"][1]
        for label in np.unique(labels):
            assert not D.directed_edge_balance(run.got["faces"][:t][run.got["labels"][:t] == label])


def test_short_output_capacities_on_a_body(ctx):
    vertices, _, faces, face_labels, _ = R.extracted("junction")
    check_variants(ctx, vertices, faces, M.cluster_grid((14, 14, 14), 2), face_labels, "junction, cell 2")


def test_a_truncated_input(ctx):
    vertices, _, faces, face_labels, _ = R.extracted("junction")
    nv, nt = len(vertices) - 300, len(faces) - 500
    assert (faces[:nt] >= nv).any()
    counts = [len(faces), nt, len(vertices), nv]
    run = check_variants(ctx, vertices, faces, M.cluster_grid((14, 14, 14), 2), face_labels, "junction, truncated", counts=counts)
    assert (run.got["map"][nv:].view(np.uint8) == FILL).all()        # rows past nv are not written
    # counts above the capacities: the capacities bound
    Run(ctx, vertices[:nv], faces[:nt], M.cluster_grid((14, 14, 14), 2), counts=[1 << 40, 1 << 33, 1 << 40, 1 << 33], face_labels=face_labels[:nt],
        what="counts above the capacities").check()
    for counts in ([0, 0, len(vertices), len(vertices)], [len(faces), len(faces), 0, 0], [0, 0, 0, 0]):
        run = Run(ctx, vertices, faces, M.cluster_grid((14, 14, 14), 2), counts=counts, face_labels=face_labels, what="counts %s" % counts).check()
        assert run.got["counts"].tolist() == [0, 0, 0, 0]
    empty = np.zeros((0, 3))
    Run(ctx, empty, empty, M.cluster_grid((4, 4, 4), 2), what="no capacities").check()
    Run(ctx, vertices, empty, M.cluster_grid((14, 14, 14), 2), what="no faces").check()


# ---- the output is a mesh again -----------------------------------------------------------------------------------------------------------------
def test_the_output_feeds_adjacency_normals_and_a_second_decimation(ctx):
    vertices, _, faces, face_labels, _ = R.extracted("split ball")
    d_vert = torch.from_numpy(np.array(vertices)).cuda()
    d_faces = torch.from_numpy(faces.astype(np.uint32).view(np.int32)).cuda().view(torch.uint32)
    d_labels = torch.from_numpy(np.array(face_labels).view(np.int32)).cuda().view(torch.uint32)
    g1, g2 = M.cluster_grid((24, 24, 24), 2), M.cluster_grid((24, 24, 24), (4, 6, 5))
    v1, f1, l1, c1, m1 = M.decimate(ctx, d_vert, d_faces, face_labels=d_labels, cell=g1[1], origin=g1[0], grid=g1[2])        # sized by the input: counts below the capacities
    adjacency = M.build_adjacency(ctx, v1, f1, c1)
    n1 = M.vertex_normals(ctx, v1, f1, c1, face_labels=l1, label=2, adjacency=adjacency)
    s1 = M.smooth(ctx, v1, f1, c1, iterations=2, adjacency=adjacency)
    v2, f2, l2, c2, m2 = M.decimate(ctx, s1, f1, c1, face_labels=l1, cell=g2[1], origin=g2[0], grid=g2[2])
    torch.cuda.synchronize()
    w1 = D.decimate_np(vertices, faces, *g1, face_labels=face_labels)
    counts1 = [len(w1["faces"]), len(w1["faces"]), len(w1["vertices"]), len(w1["vertices"])]
    assert c1.cpu().tolist() == counts1 and tuple(v1.shape) == vertices.shape and tuple(f1.shape) == faces.shape
    same_u32(v1.cpu().numpy()[:counts1[2]], w1["vertices"], "first: vertices")
    same_u32(f1.cpu().numpy()[:counts1[0]], w1["faces"].astype(np.uint32), "first: faces")
    same_u32(l1.cpu().numpy()[:counts1[0]], w1["labels"], "first: labels")
    same_u32(m1.cpu().numpy(), w1["vertex_map"], "first: map")
    same_u32(n1.cpu().numpy()[:counts1[2]], R.vertex_normals_np(w1["vertices"], w1["faces"], w1["labels"], 2), "normals of the decimated mesh")
    smoothed = R.smooth_np(w1["vertices"], w1["faces"], R.taubin(0.5, -0.53, 2))
    same_u32(s1.cpu().numpy()[:counts1[2]], smoothed, "the decimated mesh smoothed")
    w2 = D.decimate_np(smoothed, w1["faces"], *g2, face_labels=w1["labels"])
    assert 0 < len(w2["faces"]) < len(w1["faces"])
    assert c2.cpu().tolist() == [len(w2["faces"]), len(w2["faces"]), len(w2["vertices"]), len(w2["vertices"])]
    same_u32(v2.cpu().numpy()[:len(w2["vertices"])], w2["vertices"], "second: vertices")
    same_u32(f2.cpu().numpy()[:len(w2["faces"])], w2["faces"].astype(np.uint32), "second: faces")
    same_u32(l2.cpu().numpy()[:len(w2["faces"])], w2["labels"], "second: labels")
    same_u32(m2.cpu().numpy()[:counts1[2]], w2["vertex_map"], "second: map")
    assert (m2.cpu().numpy()[counts1[2]:] == D.NONE).all()
    for label in (1, 2):
        assert not D.directed_edge_balance(w2["faces"][w2["labels"] == label])


# ---- determinism and capture ------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes(ctx):
    vertices, _, faces, face_labels, _ = R.extracted("split ball")
    grid = M.cluster_grid((24, 24, 24), 3)
    runs = [Run(ctx, vertices, faces, grid, face_labels=face_labels, what="split ball").check().got for _ in range(2)]
    for k in runs[0]:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    # the vertices' order does not matter to the sums either: the mesh renumbered backwards gives the same positions and the same faces
    back = len(vertices) - 1 - faces
    other = Run(ctx, vertices[::-1], back, grid, face_labels=face_labels, what="split ball, renumbered").check().got
    assert other["vertices"].tobytes() == runs[0]["vertices"].tobytes() and other["faces"].tobytes() == runs[0]["faces"].tobytes()


def test_captured_into_a_graph_and_replayed_on_moved_vertices(ctx):
    vertices, _, faces, face_labels, _ = R.extracted("junction")
    cv, ct = len(vertices), len(faces)
    origin, cell, n = M.cluster_grid((14, 14, 14), 2)
    d_vert = torch.from_numpy(np.array(vertices)).cuda()
    d_idx = torch.from_numpy(faces.astype(np.uint32).view(np.int32)).cuda()
    d_tl = torch.from_numpy(face_labels.view(np.int32)).cuda()
    d_counts = torch.tensor([ct, ct, cv, cv], dtype=torch.int64).cuda()
    d_scratch = torch.empty((M.decimate_scratch_bytes(cv, ct, n) // 8,), dtype=torch.int64, device="cuda")
    o_vert, o_idx, o_tl = torch.empty_like(d_vert), torch.empty_like(d_idx), torch.empty_like(d_tl)
    o_map = torch.empty((cv,), dtype=torch.int32, device="cuda")
    o_counts = torch.empty((4,), dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()

    def call():
        ctx.check(ctx.mesh_decimate_rc(d_vert.data_ptr(), d_idx.data_ptr(), d_tl.data_ptr(), cv, ct, d_counts.data_ptr(), origin, cell, abi.Extent3D(*n),
                                       d_scratch.data_ptr(), o_vert.data_ptr(), cv, o_idx.data_ptr(), o_tl.data_ptr(), ct, o_map.data_ptr(), o_counts.data_ptr(),
                                       s.cuda_stream))

    torch.cuda.synchronize()
    with torch.cuda.stream(s):  # one direct call on the capture stream
        call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    torch.cuda.synchronize()
    for seed in (1, 2):
        positions = (vertices + np.random.default_rng(seed).random(vertices.shape, np.float32) * np.float32(1.5)).astype(np.float32)
        d_vert.copy_(torch.from_numpy(positions))
        d_scratch.fill_(-1)
        for t in (o_vert, o_idx, o_tl, o_map, o_counts):
            t.view(torch.uint8).fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        want = D.decimate_np(positions, faces, origin, cell, n, face_labels=face_labels)
        expect = expected(want, cv, cv, cv, ct, True, True)
        assert o_counts.cpu().tolist() == expect["counts"].tolist()
        same_u32(o_vert.cpu().numpy(), expect["vertices"], "replay %d: vertices" % seed)
        same_u32(o_idx.cpu().numpy().view(np.uint32), expect["faces"], "replay %d: faces" % seed)
        same_u32(o_tl.cpu().numpy().view(np.uint32), expect["labels"], "replay %d: labels" % seed)
        same_u32(o_map.cpu().numpy().view(np.uint32), expect["map"], "replay %d: map" % seed)


# ---- rejected calls -----------------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing(ctx):
    vertices, faces = R.small_meshes()["tetrahedron"]
    cv, ct, n = 4, 4, (4, 4, 4)
    # [vertices 48 | indices 48 | labels 16 | counts 32 | out vertices 48 | out indices 48 | out labels 16 | map 16 | out counts 32 | scratch], each at a multiple of 64
    out = torch.full((8192,), FILL, dtype=torch.uint8, device="cuda")
    a = out.data_ptr()
    assert a % 8 == 0 and M.decimate_scratch_bytes(cv, ct, n) <= 8192 - 1024
    ok = dict(vert=a, idx=a + 64, tl=a + 128, counts=a + 192, overt=a + 256, oidx=a + 320, otl=a + 384, map=a + 448, ocounts=a + 512, scratch=a + 1024, cv=cv, ct=ct,
              ocv=cv, oct=ct, origin=(0.0, 0.0, 0.0), cell=(0.5, 0.5, 0.5), grid=n)
    out[0:48] = torch.from_numpy(vertices.view(np.uint8).reshape(-1)).cuda()
    out[64:112] = torch.from_numpy(faces.astype(np.uint32).view(np.uint8).reshape(-1)).cuda()
    out[128:144] = torch.from_numpy(np.array([5, 6, 7, 8], np.uint32).view(np.uint8)).cuda()
    out[192:224] = torch.from_numpy(np.array([ct, ct, cv, cv], np.int64).view(np.uint8)).cuda()
    before = out.clone()
    bad, unsupported, big, inf, nan = abi.VKV_E_INVALID_ARGUMENT, abi.VKV_E_UNSUPPORTED, 1 << 32, float("inf"), float("nan")

    def call(**change):
        k = dict(ok, **change)
        return ctx.mesh_decimate_rc(k["vert"], k["idx"], k["tl"], k["cv"], k["ct"], k["counts"], k["origin"], k["cell"], abi.Extent3D(*k["grid"]), k["scratch"],
                                    k["overt"], k["ocv"], k["oidx"], k["otl"], k["oct"], k["map"], k["ocounts"], st())

    for name in ("vert", "idx", "counts", "origin", "cell", "scratch", "ocounts"):
        assert call(**{name: None}) == bad and "null" in ctx.last_error(), name
    for name in ("vert", "idx", "tl", "overt", "oidx", "otl", "map"):
        assert call(**{name: ok[name] + 2}) == bad and "4-byte" in ctx.last_error(), name
    for name in ("counts", "scratch", "ocounts"):
        assert call(**{name: ok[name] + 4}) == bad and "8-byte" in ctx.last_error(), name
    for grid in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        assert call(grid=grid) == bad and "grid" in ctx.last_error(), grid
    for c in (0.0, -1.0, inf, nan):
        for axis in range(3):
            assert call(cell=tuple(c if i == axis else 0.5 for i in range(3))) == bad and "grid_cell[%d]" % axis in ctx.last_error(), (c, axis)
    for o in (inf, -inf, nan):
        for axis in range(3):
            assert call(origin=tuple(o if i == axis else 0.0 for i in range(3))) == bad and "grid_origin[%d]" % axis in ctx.last_error(), (o, axis)
    for o in ("overt", "oidx", "otl", "map", "ocounts"):
        for i in ("vert", "idx", "tl", "counts", "scratch") + tuple(p for p in ("overt", "oidx", "otl", "map", "ocounts") if p != o):
            assert call(**{o: ok[i]}) == bad and "of its own" in ctx.last_error(), (o, i)
    for change in (dict(overt=None), dict(oidx=None), dict(otl=None)):
        assert call(**change) == bad and "capacity" in ctx.last_error(), change
    for name in ("cv", "ct", "ocv", "oct"):
        assert call(**{name: big}) == unsupported and "2^32" in ctx.last_error(), name
    for grid in ((65536, 65536, 1), (1, 65536, 65536), (0xffffffff, 2, 1), (0xffffffff, 0xffffffff, 0xffffffff)):
        assert call(grid=grid) == unsupported and "cells" in ctx.last_error(), grid
        assert lib.load().vkv_mesh_decimate_scratch_bytes(cv, ct, abi.Extent3D(*grid)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    # and the accepted calls next to them: no labels with a NULL d_out_triangle_labels, zero capacities with NULL outputs, then the full call
    assert call(tl=None, otl=None, map=None) == abi.VKV_OK and call(overt=None, oidx=None, otl=None, ocv=0, oct=0) == abi.VKV_OK and call() == abi.VKV_OK
    torch.cuda.synchronize()
    want = D.decimate_np(vertices, faces, ok["origin"], ok["cell"], n, face_labels=np.array([5, 6, 7, 8], np.uint32))
    assert len(want["faces"]) == 4 and out[512:544].cpu().numpy().view(np.int64).tolist() == [4, 4, 4, 4]
    same_u32(out[256:304].cpu().numpy().view(np.float32).reshape(4, 3), want["vertices"], "the accepted call: vertices")
    same_u32(out[320:368].cpu().numpy().view(np.uint32).reshape(4, 3), want["faces"].astype(np.uint32), "faces")
    same_u32(out[384:400].cpu().numpy().view(np.uint32), want["labels"], "labels")
    same_u32(out[448:464].cpu().numpy().view(np.uint32), want["vertex_map"], "map")
    for lo, hi in ((304, 320), (368, 384), (400, 448), (464, 512), (544, 1024)):
        assert bool((out[lo:hi] == FILL).all()), (lo, hi)
    assert torch.equal(out[:256], before[:256])


# ---- vkvolume_amd.mesh ----------------------------------------------------------------------------------------------------------------------------
def test_mesh_decimate_equals_the_c_call(ctx):
    vertices, _, faces, face_labels, _ = R.extracted("junction")
    d_vert = torch.from_numpy(np.array(vertices)).cuda()
    d_faces = torch.from_numpy(faces.astype(np.uint32).view(np.int32)).cuda().view(torch.uint32)
    d_labels = torch.from_numpy(face_labels.view(np.int32)).cuda().view(torch.uint32)
    origin, cell, n = M.cluster_grid((14, 14, 14), (2, 3, 5))
    direct = Run(ctx, vertices, faces, (origin, cell, n), face_labels=face_labels, what="junction").check()
    v, f, labels, counts, vmap = M.decimate(ctx, d_vert, d_faces, face_labels=d_labels, cell=(2, 3, 5), origin=origin, grid=n)
    assert v.dtype == torch.float32 and f.dtype == torch.uint32 and labels.dtype == torch.uint32 and vmap.dtype == torch.uint32 and counts.dtype == torch.int64
    assert tuple(v.shape) == vertices.shape and tuple(f.shape) == faces.shape and tuple(vmap.shape) == (len(vertices),)
    t, _, nv, _ = counts.cpu().tolist()
    assert [t, t, nv, nv] == direct.got["counts"].tolist()
    same_u32(v.cpu().numpy()[:nv], direct.got["vertices"][:nv], "vertices")
    same_u32(f.cpu().numpy()[:t], direct.got["faces"][:t].view(np.uint32), "faces")
    same_u32(labels.cpu().numpy()[:t], direct.got["labels"][:t].view(np.uint32), "labels")
    same_u32(vmap.cpu().numpy(), direct.got["map"].view(np.uint32), "map")
    assert not v.cpu().numpy()[nv:].any() and not f.cpu().numpy()[t:].any()        # rows past the counts are zero
    same_u32(d_vert.cpu().numpy(), vertices, "the input stays")
    # without labels; with capacities; a grid derived from the vertices
    v2, f2, none, counts2, _ = M.decimate(ctx, d_vert, d_faces, cell=(2, 3, 5), origin=origin, grid=abi.Extent3D(*n), capacity=(nv - 5, t - 7))
    assert none is None and counts2.cpu().tolist() == [t, t - 7, nv, nv - 5] and tuple(v2.shape) == (nv - 5, 3) and tuple(f2.shape) == (t - 7, 3)
    same_u32(v2.cpu().numpy(), direct.got["vertices"][:nv - 5], "short: vertices")
    same_u32(f2.cpu().numpy(), direct.got["faces"][:t - 7].view(np.uint32), "short: faces")
    v3, f3, _, counts3, _ = M.decimate(ctx, d_vert, d_faces, cell=2.0)
    want = D.decimate_np(vertices, faces, *D.grid_for(vertices, 2.0))
    assert counts3.cpu().tolist() == [len(want["faces"]), len(want["faces"]), len(want["vertices"]), len(want["vertices"])]
    same_u32(v3.cpu().numpy()[:len(want["vertices"])], want["vertices"], "derived grid: vertices")
    empty = M.decimate(ctx, d_vert[:0], d_faces[:0], cell=2.0)
    assert tuple(empty[0].shape) == (0, 3) and tuple(empty[1].shape) == (0, 3) and empty[3].cpu().tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        M.decimate(ctx, d_vert.cpu(), d_faces)
    with pytest.raises(ValueError):
        M.decimate(ctx, d_vert, d_faces, face_labels=d_labels[:-1])
    with pytest.raises(ValueError):
        M.decimate(ctx, d_vert, d_faces, origin=(0, 0, 0))
    with pytest.raises(ValueError):        # rows past the counts are not positions: no grid is derived from them
        M.decimate(ctx, d_vert, d_faces, counts=counts)
    with pytest.raises(ValueError):
        M.decimate(ctx, d_vert, d_faces, grid=(0, 1, 1))
    with pytest.raises(lib.VkvError):
        M.decimate(ctx, d_vert, d_faces, cell=float("nan"), grid=(2, 2, 2))
