"""GPU: vkv_mesh_adjacency, vkv_mesh_smooth and vkv_mesh_vertex_normals bit for bit against the numpy statement of
tests/mesh_smooth_ref.py: every float of the smoothed vertices after 0, 1, 2 and 5 passes (both ping-pong parities end in d_vertices) and
after ten Taubin iterations, every float of the normals over all faces and per label.

The meshes: a tetrahedron, one with an isolated vertex (k = 0), three faces on one edge, a face repeated with reversed winding, faces that
hold a vertex twice, fans of 16, 17 and 100 triangles about one vertex (the build sorts up to 16 faces of a vertex in LDS and more where
they lie; 100 is a segment longer than a wave), and from the label extractor's statement a
radius-9 ball split into two labels, a junction of three labels (thousands of vertices: several workgroups and, with 4142 vertices, a second
scan chunk) and a body that leaves the box.  Counts below the capacities make faces name vertices at or past nv; those faces are not used.
One test takes its mesh straight from vkv_label_mesh_indexed with capacities below the totals and never reads the counts on the host.

Every buffer is a tests/helpers.py guarded() allocation, pre-filled and compared as a whole: rows past nv must keep their bits in
d_vertices, d_swap and d_normals, and all guards must be intact, so nothing here relies on, or can cause, a fault."""
import numpy as np
import pytest
import torch

from tests import helpers as T
from tests import mesh_smooth_ref as R
from tests.test_label_mesh_indexed_cpu import label_indexed_np
from vkvolume_amd import abi, labels as LB, lib, mesh as M

pytestmark = pytest.mark.gpu
FILL = 0xA5
TAUBIN = R.taubin(0.5, -0.53, 10)
PASSES = {0: [], 1: [0.5], 2: [0.5, -0.53], 5: [0.5, -0.53, 0.5, -0.53, 0.3]}


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


def prefilled(shape, dtype=np.float32):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


class DeviceMesh:
    """a mesh in guarded device buffers with its adjacency built: vertices [cv, 3], faces [ct, 3], counts [4]; cv and ct are the capacities"""

    def __init__(self, ctx, vertices, faces, counts=None, face_labels=None, what=""):
        self.ctx, self.what = ctx, what
        self.h_vertices = np.array(vertices, np.float32)        # a copy: the shared meshes are read-only
        self.h_faces = np.ascontiguousarray(faces).astype(np.int64)
        self.cv, self.ct = len(self.h_vertices), len(self.h_faces)
        self.h_counts = [self.ct, self.ct, self.cv, self.cv] if counts is None else [int(c) for c in counts]
        self.nv, self.nt = R.bounds(self.cv, self.ct, self.h_counts)
        self.h_labels = None if face_labels is None else np.array(face_labels, np.uint32)
        self.handles = []
        self.vertices = self.buffer("d_vertices", self.h_vertices if self.cv else (1, 3), np.float32)
        self.faces = self.buffer("d_indices", self.h_faces.astype(np.uint32).view(np.int32) if self.ct else (1, 3), np.int32)
        self.labels = None if face_labels is None else self.buffer("d_triangle_labels", self.h_labels.view(np.int32) if self.ct else (1,), np.int32)
        self.counts = self.buffer("d_counts", np.array(self.h_counts, np.int64), np.int64)
        nbytes = M.adjacency_scratch_bytes(self.cv, self.ct)
        assert nbytes == lib.load().vkv_mesh_adjacency_scratch_bytes(self.cv, self.ct) and nbytes % 8 == 0
        self.adjacency = self.buffer("d_adjacency", (nbytes // 8,), np.int64)
        self.swap = self.buffer("d_swap", (max(self.cv, 1), 3), np.float32)
        self.normals = self.buffer("d_normals", (max(self.cv, 1), 3), np.float32)
        ctx.check(ctx.mesh_adjacency_rc(self.faces.data_ptr(), self.ct, self.cv, self.counts.data_ptr(), self.adjacency.data_ptr(), st()))

    def buffer(self, name, array_or_shape, dtype):
        view, handle = T.guarded(array_or_shape, 0, FILL, "cuda", dtype=dtype)
        self.handles.append((name, handle))
        return view

    def reset(self, vertices=None):
        self.vertices[:self.cv].copy_(torch.from_numpy(self.h_vertices if vertices is None else np.ascontiguousarray(vertices, np.float32)))

    def smooth(self, factors, pinned=None):
        """the whole d_vertices after the passes, from the mesh's own positions"""
        self.reset()
        d_pinned = None if pinned is None else self.buffer("d_pinned", np.ascontiguousarray(pinned, np.uint8), np.uint8)
        self.ctx.check(self.ctx.mesh_smooth_rc(self.vertices.data_ptr(), self.swap.data_ptr(), self.cv, self.counts.data_ptr(), self.adjacency.data_ptr(),
                                               None if d_pinned is None else d_pinned.data_ptr(), [float(f) for f in factors], st()))
        torch.cuda.synchronize()
        self.check_guards()
        swap = self.swap.cpu().numpy()
        assert (swap[self.nv:].view(np.uint8) == FILL).all(), "%s: d_swap was written past nv" % self.what
        return self.vertices.cpu().numpy()

    def vertex_normals(self, label=None):
        """the whole d_normals, pre-filled, of the positions now in d_vertices; label None: no filter"""
        self.normals.view(torch.uint8).fill_(FILL)
        self.ctx.check(self.ctx.mesh_vertex_normals_rc(self.vertices.data_ptr(), self.faces.data_ptr(), None if label is None else self.labels.data_ptr(),
                                                       0 if label is None else label, self.cv, self.ct, self.counts.data_ptr(), self.adjacency.data_ptr(),
                                                       self.normals.data_ptr(), st()))
        torch.cuda.synchronize()
        self.check_guards()
        return self.normals.cpu().numpy()

    def check_guards(self):
        for name, h in self.handles:
            changed = h.buf.cpu().numpy() != h.fill
            changed[h.start:h.stop] = False
            bad = np.flatnonzero(changed).tolist()
            assert not bad, "%s: %s: guard bytes %s changed (payload is bytes %d .. %d)" % (self.what, name, bad[:8], h.start, h.stop - 1)
        assert np.array_equal(self.faces.cpu().numpy().view(np.uint32)[:self.ct], self.h_faces.astype(np.uint32)[:self.ct]), "%s: the indices changed" % self.what
        assert self.counts.cpu().tolist() == self.h_counts, "%s: the counts changed" % self.what

    def want_smooth(self, factors, pinned=None):
        return R.smooth_np(self.h_vertices, self.h_faces, factors, counts=self.h_counts, pinned=pinned)

    def want_normals(self, positions, label=None):
        want = prefilled((max(self.cv, 1), 3))
        want[:self.nv] = R.vertex_normals_np(positions, self.h_faces, None if label is None else self.h_labels, 0 if label is None else label,
                                             counts=self.h_counts)
        return want

    def check_all(self, passes=PASSES, labels=()):
        for n, factors in passes.items():
            got = self.smooth(factors)
            want = self.want_smooth(factors)
            same_u32(got[:self.cv], want, "%s: %s passes" % (self.what, n))
            same_u32(got[self.nv:self.cv], self.h_vertices[self.nv:], "%s: %s passes, rows past nv" % (self.what, n))
            for label in (None,) + tuple(labels):
                same_u32(self.vertex_normals(label), self.want_normals(want, label), "%s: %s passes, normals, label %s" % (self.what, n, label))


# ---- the hand-made meshes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.small_meshes()))
def test_small_meshes(ctx, name):
    vertices, faces = R.small_meshes()[name]
    mesh = DeviceMesh(ctx, vertices, faces, face_labels=1 + np.arange(len(faces)) % 2, what=name)
    mesh.check_all(labels=(1, 2))
    moved = mesh.want_smooth(PASSES[5])
    if name == "isolated vertex":
        assert np.array_equal(moved[4], vertices[4]) and not np.array_equal(moved[:4], vertices[:4])
    else:
        assert not (moved == vertices).all(axis=1).any()        # every vertex has a neighbour and moves


def test_faces_that_name_vertices_past_nv_are_not_used(ctx):
    vertices, faces = R.small_meshes()["fan of 100"]
    # 101 vertices, 60 of them meant: the fan's triangles 59 .. 99 name a vertex at or past nv; and of 100 triangles 80 are meant
    mesh = DeviceMesh(ctx, vertices, faces, counts=[1000, 80, 7000, 60], what="fan, nv 60, nt 80")
    assert (mesh.nv, mesh.nt) == (60, 80) and len(R.used_faces(faces, 60, 80)[0]) == 58
    mesh.check_all()
    # counts above the capacities: the capacities bound
    mesh = DeviceMesh(ctx, vertices[:60], faces[:80], counts=[1000, 1000, 7000, 7000], what="fan, capacities 60 and 80")
    assert (mesh.nv, mesh.nt) == (60, 80)
    mesh.check_all()
    same_u32(mesh.want_smooth(TAUBIN), R.smooth_np(vertices, faces, TAUBIN, counts=[1000, 80, 7000, 60])[:60], "the two statements of the same cut")
    for counts in ([0, 0, 101, 101], [100, 100, 0, 0], [0, 0, 0, 0]):        # no faces, no vertices
        mesh = DeviceMesh(ctx, vertices, faces, counts=counts, what="fan, counts %s" % counts)
        mesh.check_all(passes={2: PASSES[2]})
        same_u32(mesh.want_smooth(PASSES[2]), vertices, "nothing moves")


def test_empty_capacities(ctx):
    for vertices, faces in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)), (R.small_meshes()["tetrahedron"][0], np.zeros((0, 3), np.int64))):
        mesh = DeviceMesh(ctx, vertices, faces, what="%d vertices, no faces" % len(vertices))
        mesh.check_all(passes={1: PASSES[1]})


# ---- the extractor's meshes -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["split ball", "junction"])
def body_mesh(ctx, request):
    vertices, pairs, faces, face_labels, _ = R.extracted(request.param)
    assert len(vertices) > 4096 and len(faces) > 9000
    return DeviceMesh(ctx, vertices, faces, face_labels=face_labels, what=request.param)


def test_bodies_every_pass_count_and_every_label(ctx, body_mesh):
    body_mesh.check_all(labels=(1, 2, 3))


def test_bodies_ten_taubin_iterations_and_interface_normals(ctx, body_mesh):
    got = body_mesh.smooth(TAUBIN)
    want = body_mesh.want_smooth(TAUBIN)
    same_u32(got, want, body_mesh.what + ": ten Taubin iterations")
    every, one, two = (body_mesh.vertex_normals(label) for label in (None, 1, 2))
    same_u32(every, body_mesh.want_normals(want), body_mesh.what + ": normals of the smoothed mesh")
    if body_mesh.what == "split ball":
        from tests.test_mesh_smooth_cpu import interior_interface
        inside = interior_interface(R.extracted("split ball")[1], body_mesh.h_faces)
        assert inside.sum() > 800 and not every[inside].any() and np.array_equal(one[inside], -two[inside]) and (one[inside, 0] > 1).all()


def test_counts_below_the_capacities_on_a_body(ctx):
    vertices, _, faces, face_labels, _ = R.extracted("junction")
    nv, nt = len(vertices) - 300, len(faces) - 500
    mesh = DeviceMesh(ctx, vertices, faces, counts=[len(faces), nt, len(vertices), nv], face_labels=face_labels, what="junction, truncated")
    assert (faces[:nt] >= nv).any()
    mesh.check_all(passes={2: PASSES[2], 5: PASSES[5]}, labels=(2,))


def test_pinned_rim_of_a_body_that_leaves_the_box(ctx):
    vertices, _, faces, face_labels, _ = R.extracted("box cut")
    rim = M.boundary_vertices(faces, len(vertices))
    assert 20 < rim.sum() < len(rim)
    mesh = DeviceMesh(ctx, vertices, faces, face_labels=face_labels, what="box cut")
    for factors in (PASSES[1], TAUBIN):
        got, want = mesh.smooth(factors, pinned=rim), mesh.want_smooth(factors, pinned=rim)
        same_u32(got, want, "box cut, pinned, %d passes" % len(factors))
        same_u32(got[rim], vertices[rim], "the rim stays")
        assert not np.array_equal(mesh.want_smooth(factors)[rim], vertices[rim])        # and would have moved
    same_u32(mesh.smooth(TAUBIN, pinned=np.where(rim, 0x80, 0).astype(np.uint8)), mesh.want_smooth(TAUBIN, pinned=rim), "any non-zero byte pins")
    same_u32(mesh.smooth(TAUBIN, pinned=np.ones(len(rim), np.uint8)), vertices, "everything pinned")


def test_straight_from_the_label_extractor_with_short_capacities(ctx):
    """vkv_label_mesh_indexed into buffers shorter than the totals, then adjacency, smoothing and normals: the counts never leave the device"""
    labels = R.split_ball_labels()
    wv, _, _, wf, wl = label_indexed_np(labels)
    cap_v, cap_t = len(wv) - 700, len(wf) - 900
    d, h, w = labels.shape
    e = abi.Extent3D(w, h, d)
    d_lab = torch.from_numpy(labels.view(np.int32)).cuda()
    d_scratch = torch.empty((LB.mesh_indexed_scratch_bytes(e) // 8,), dtype=torch.int64, device="cuda")
    d_vert, h_vert = T.guarded((cap_v, 3), 0, FILL, "cuda", dtype=np.float32)
    d_idx, h_idx = T.guarded((cap_t, 3), 0, FILL, "cuda", dtype=np.int32)
    d_tl, h_tl = T.guarded((cap_t,), 0, FILL, "cuda", dtype=np.int32)
    d_counts, h_counts = T.guarded((4,), 0, FILL, "cuda", dtype=np.int64)
    d_adj, h_adj = T.guarded((M.adjacency_scratch_bytes(cap_v, cap_t) // 8,), 0, FILL, "cuda", dtype=np.int64)
    d_swap, h_swap = T.guarded((cap_v, 3), 0, FILL, "cuda", dtype=np.float32)
    d_norm, h_norm = T.guarded((cap_v, 3), 0, FILL, "cuda", dtype=np.float32)
    ctx.check(ctx.label_mesh_indexed_rc(d_lab.data_ptr(), e, None, None, 0, None, 0.0, None, None, d_scratch.data_ptr(), d_vert.data_ptr(), None, None, cap_v,
                                        d_idx.data_ptr(), d_tl.data_ptr(), cap_t, d_counts.data_ptr(), st()))
    ctx.check(ctx.mesh_adjacency_rc(d_idx.data_ptr(), cap_t, cap_v, d_counts.data_ptr(), d_adj.data_ptr(), st()))
    ctx.check(ctx.mesh_smooth_rc(d_vert.data_ptr(), d_swap.data_ptr(), cap_v, d_counts.data_ptr(), d_adj.data_ptr(), None, [float(f) for f in TAUBIN[:5]], st()))
    ctx.check(ctx.mesh_vertex_normals_rc(d_vert.data_ptr(), d_idx.data_ptr(), d_tl.data_ptr(), 2, cap_v, cap_t, d_counts.data_ptr(), d_adj.data_ptr(),
                                         d_norm.data_ptr(), st()))
    torch.cuda.synchronize()
    counts = [len(wf), cap_t, len(wv), cap_v]
    assert d_counts.cpu().tolist() == counts
    same_u32(d_idx.cpu().numpy().view(np.uint32), wf[:cap_t].astype(np.uint32), "the extractor's indices")
    assert (wf[:cap_t] >= cap_v).any()
    want = R.smooth_np(wv[:cap_v], wf[:cap_t], TAUBIN[:5], counts=counts)
    same_u32(d_vert.cpu().numpy(), want, "smoothed")
    same_u32(d_norm.cpu().numpy(), R.vertex_normals_np(want, wf[:cap_t], wl[:cap_t], 2, counts=counts), "normals of label 2")
    for name, handle in (("d_vertices", h_vert), ("d_indices", h_idx), ("d_triangle_labels", h_tl), ("d_counts", h_counts), ("d_adjacency", h_adj),
                         ("d_swap", h_swap), ("d_normals", h_norm)):
        assert not handle.check(), name


# ---- determinism and capture ------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes(ctx):
    vertices, _, faces, face_labels, _ = R.extracted("junction")
    runs = []
    for _ in range(2):
        mesh = DeviceMesh(ctx, vertices, faces, face_labels=face_labels, what="junction")
        smoothed = mesh.smooth(TAUBIN)
        runs.append((mesh.adjacency.cpu().numpy().tobytes(), smoothed.tobytes(), mesh.vertex_normals(3).tobytes()))
    assert runs[0] == runs[1]
    # the adjacency does not depend on the order of the faces either, once its face numbers are set aside: the smoothed bytes agree
    order = np.random.default_rng(3).permutation(len(faces))
    mesh = DeviceMesh(ctx, vertices, faces[order], face_labels=face_labels[order], what="junction, permuted")
    assert mesh.smooth(TAUBIN).tobytes() == runs[0][1] and mesh.vertex_normals(3).tobytes() == runs[0][2]


def test_captured_into_a_graph_and_replayed_on_new_positions(ctx):
    vertices, _, faces, face_labels, _ = R.extracted("split ball")
    cv, ct = len(vertices), len(faces)
    d_vert = torch.from_numpy(np.array(vertices)).cuda()
    d_idx = torch.from_numpy(faces.astype(np.uint32).view(np.int32)).cuda()
    d_tl = torch.from_numpy(face_labels.view(np.int32)).cuda()
    d_counts = torch.tensor([ct, ct, cv, cv], dtype=torch.int64).cuda()
    d_adj = torch.empty((M.adjacency_scratch_bytes(cv, ct) // 8,), dtype=torch.int64, device="cuda")
    d_swap, d_norm = torch.empty_like(d_vert), torch.empty_like(d_vert)
    s = torch.cuda.Stream()
    factors = [float(f) for f in TAUBIN[:3]]        # an odd number of passes: the copy back is part of the graph

    def call():
        ctx.check(ctx.mesh_adjacency_rc(d_idx.data_ptr(), ct, cv, d_counts.data_ptr(), d_adj.data_ptr(), s.cuda_stream))
        ctx.check(ctx.mesh_smooth_rc(d_vert.data_ptr(), d_swap.data_ptr(), cv, d_counts.data_ptr(), d_adj.data_ptr(), None, factors, s.cuda_stream))
        ctx.check(ctx.mesh_vertex_normals_rc(d_vert.data_ptr(), d_idx.data_ptr(), d_tl.data_ptr(), 1, cv, ct, d_counts.data_ptr(), d_adj.data_ptr(),
                                             d_norm.data_ptr(), s.cuda_stream))

    torch.cuda.synchronize()
    with torch.cuda.stream(s):  # one direct call on the capture stream
        call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    torch.cuda.synchronize()
    for seed in (1, 2):
        positions = (vertices + np.random.default_rng(seed).random(vertices.shape, np.float32) * np.float32(0.25)).astype(np.float32)
        d_vert.copy_(torch.from_numpy(positions))
        d_adj.fill_(-1)
        d_swap.view(torch.uint8).fill_(FILL)
        d_norm.view(torch.uint8).fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        want = R.smooth_np(positions, faces, factors)
        same_u32(d_vert.cpu().numpy(), want, "replay %d: vertices" % seed)
        same_u32(d_norm.cpu().numpy(), R.vertex_normals_np(want, faces, face_labels, 1), "replay %d: normals" % seed)


# ---- rejected calls ---------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing(ctx):
    vertices, faces = R.small_meshes()["tetrahedron"]
    cv, ct = 4, 4
    # [vertices 48 | swap 48 | normals 48 | indices 48 | triangle labels 16 | counts 32 | pinned 8 | adjacency], each at a multiple of 64
    out = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    a = out.data_ptr()
    assert a % 8 == 0 and M.adjacency_scratch_bytes(cv, ct) <= 4096 - 512
    ok = dict(vert=a, swap=a + 64, norm=a + 128, idx=a + 192, tl=a + 256, counts=a + 320, pinned=a + 384, adj=a + 512, cv=cv, ct=ct, factors=[0.5, -0.53], label=1)
    out[0:48] = torch.from_numpy(vertices.view(np.uint8).reshape(-1)).cuda()
    out[192:240] = torch.from_numpy(faces.astype(np.uint32).view(np.uint8).reshape(-1)).cuda()
    out[320:352] = torch.from_numpy(np.array([ct, ct, cv, cv], np.int64).view(np.uint8)).cuda()
    before = out.clone()
    bad, big, inf, nan = abi.VKV_E_INVALID_ARGUMENT, 1 << 32, float("inf"), float("nan")

    def adjacency(**change):
        k = dict(ok, **change)
        return ctx.mesh_adjacency_rc(k["idx"], k["ct"], k["cv"], k["counts"], k["adj"], st())

    def smooth(**change):
        k = dict(ok, **change)
        return ctx.mesh_smooth_rc(k["vert"], k["swap"], k["cv"], k["counts"], k["adj"], k["pinned"], k["factors"], st())

    def normals(**change):
        k = dict(ok, **change)
        return ctx.mesh_vertex_normals_rc(k["vert"], k["idx"], k["tl"], k["label"], k["cv"], k["ct"], k["counts"], k["adj"], k["norm"], st())

    for name in ("idx", "counts", "adj"):
        assert adjacency(**{name: None}) == bad and "null" in ctx.last_error(), name
    assert adjacency(idx=ok["idx"] + 2) == bad and "aligned" in ctx.last_error()
    assert adjacency(counts=ok["counts"] + 4) == bad and adjacency(adj=ok["adj"] + 4) == bad and "8-byte" in ctx.last_error()
    assert adjacency(cv=big) == abi.VKV_E_UNSUPPORTED and adjacency(ct=big) == abi.VKV_E_UNSUPPORTED and "2^32" in ctx.last_error()
    for name in ("vert", "swap", "counts", "adj"):
        assert smooth(**{name: None}) == bad and "null" in ctx.last_error(), name
    assert smooth(vert=ok["vert"] + 2) == bad and smooth(swap=ok["swap"] + 1) == bad and "aligned" in ctx.last_error()
    assert smooth(counts=ok["counts"] + 4) == bad and smooth(adj=ok["adj"] + 4) == bad
    assert smooth(swap=ok["vert"]) == bad and "d_swap" in ctx.last_error()
    assert smooth(factors=(None, 2)) == bad and "factors" in ctx.last_error()
    for f in (inf, -inf, nan):
        assert smooth(factors=[0.5, f]) == bad and "finite" in ctx.last_error()
    assert smooth(cv=big) == abi.VKV_E_UNSUPPORTED
    for name in ("vert", "idx", "norm", "counts", "adj"):
        assert normals(**{name: None}) == bad and "null" in ctx.last_error(), name
    for name in ("vert", "idx", "tl", "norm"):
        assert normals(**{name: ok[name] + 2}) == bad and "aligned" in ctx.last_error(), name
    assert normals(counts=ok["counts"] + 4) == bad and normals(adj=ok["adj"] + 4) == bad
    assert normals(norm=ok["vert"]) == bad and "d_normals" in ctx.last_error()
    assert normals(cv=big) == abi.VKV_E_UNSUPPORTED and normals(ct=big) == abi.VKV_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    # and the accepted calls next to them: an odd d_pinned, zero passes with NULL factors
    out[384:392] = 0
    assert adjacency() == abi.VKV_OK and smooth(pinned=ok["pinned"] + 1) == abi.VKV_OK and smooth(factors=None) == abi.VKV_OK and normals() == abi.VKV_OK
    torch.cuda.synchronize()
    want = R.smooth_np(vertices, faces, [0.5, -0.53])
    same_u32(out[0:48].cpu().numpy().view(np.float32).reshape(4, 3), want, "the accepted call")
    same_u32(out[128:176].cpu().numpy().view(np.float32).reshape(4, 3), R.vertex_normals_np(want, faces, np.full(4, FILL * 0x01010101, np.uint32), 1), "its normals")
    assert bool((out[48:64] == FILL).all()) and bool((out[176:192] == FILL).all()) and torch.equal(out[192:384], before[192:384])


# ---- vkvolume_amd.mesh --------------------------------------------------------------------------------------------------------------------
def test_mesh_smooth_and_vertex_normals_match_the_c_calls(ctx):
    vertices, _, faces, face_labels, _ = R.extracted("box cut")
    d_vert = torch.from_numpy(np.array(vertices)).cuda()
    d_faces = torch.from_numpy(faces.astype(np.uint32).view(np.int32)).cuda().view(torch.uint32)
    d_labels = torch.from_numpy(face_labels.view(np.int32)).cuda().view(torch.uint32)
    got = M.smooth(ctx, d_vert, d_faces)
    assert got.dtype == torch.float32 and got.shape == d_vert.shape and got.data_ptr() != d_vert.data_ptr()
    want = R.smooth_np(vertices, faces, TAUBIN)
    same_u32(got.cpu().numpy(), want, "mesh.smooth defaults")
    same_u32(d_vert.cpu().numpy(), vertices, "the input stays")
    same_u32(M.smooth(ctx, d_vert, d_faces, lam=0.5, mu=None, iterations=3).cpu().numpy(), R.smooth_np(vertices, faces, [0.5] * 3), "Laplacian")
    same_u32(M.smooth(ctx, d_vert, d_faces, iterations=0).cpu().numpy(), vertices, "no iterations")
    rim = M.boundary_vertices(faces, len(vertices))
    adjacency = M.build_adjacency(ctx, d_vert, d_faces)
    for pinned in (rim, torch.from_numpy(rim).cuda(), torch.from_numpy(rim.astype(np.uint8))):
        same_u32(M.smooth(ctx, d_vert, d_faces, pinned=pinned, adjacency=adjacency).cpu().numpy(), R.smooth_np(vertices, faces, TAUBIN, pinned=rim), "pinned")
    same_u32(M.vertex_normals(ctx, got, d_faces, adjacency=adjacency).cpu().numpy(), R.vertex_normals_np(want, faces), "normals")
    same_u32(M.vertex_normals(ctx, got, d_faces, face_labels=d_labels, label=1).cpu().numpy(), R.vertex_normals_np(want, faces, face_labels, 1), "label 1")
    assert not M.vertex_normals(ctx, got, d_faces, face_labels=d_labels, label=2).cpu().numpy().any()
    # with the extraction's counts: rows past them are copies, normals there zero
    nv, nt = len(vertices) - 50, len(faces) - 70
    counts = torch.tensor([len(faces), nt, len(vertices), nv], dtype=torch.int64).cuda()
    got = M.smooth(ctx, d_vert, d_faces, counts=counts, iterations=2)
    same_u32(got.cpu().numpy(), R.smooth_np(vertices, faces, TAUBIN[:4], counts=counts.cpu().tolist()), "counts")
    n = M.vertex_normals(ctx, got, d_faces, counts=counts).cpu().numpy()
    same_u32(n[:nv], R.vertex_normals_np(got.cpu().numpy(), faces, counts=counts.cpu().tolist()), "counts: normals")
    assert not n[nv:].any()
    empty = M.smooth(ctx, d_vert[:0], d_faces[:0])
    assert tuple(empty.shape) == (0, 3) and tuple(M.vertex_normals(ctx, d_vert[:0], d_faces[:0]).shape) == (0, 3)
    with pytest.raises(ValueError):
        M.smooth(ctx, d_vert.cpu(), d_faces)
    with pytest.raises(ValueError):
        M.smooth(ctx, d_vert, d_faces.view(torch.int32).to(torch.int64))
    with pytest.raises(ValueError):
        M.smooth(ctx, d_vert, d_faces, pinned=rim[:-1])
    with pytest.raises(ValueError):
        M.smooth(ctx, d_vert, d_faces[:-1], adjacency=adjacency)
    with pytest.raises(ValueError):
        M.vertex_normals(ctx, d_vert, d_faces, face_labels=d_labels[:-1], label=1)
    with pytest.raises(lib.VkvError):
        M.smooth(ctx, d_vert, d_faces, lam=float("nan"))
