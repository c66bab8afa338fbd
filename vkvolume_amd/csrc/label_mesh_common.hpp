// label_mesh_common.hpp — what only the kernels of label_mesh.hip (vkv_label_mesh) and label_mesh_indexed.hip (vkv_label_mesh_indexed) share:
// the argument block, the row loads of labels and bytes, the table lookup that turns labels into shown labels, the triangle counts of a
// tetrahedron, a cube and a lane, the vertex rule and the argument block's builder (label_geom); DESIGN.md §5.22, §5.23.  The tiles, the
// plan, the scratch layout and every step of the pipeline that the isosurface meshes take as well are mesh_common.hpp's.
#pragma once

#include "mesh_common.hpp"
#include "mtet_table.hpp"
#include "row_loads.hpp"

namespace vkv
{

struct LabelGeom
{
	MeshGeom        G;             // the box's cubes, the tiles and the visibility map (thr = 1: a byte of 255 passes, 0 does not); vol may be null
	const uint32_t *labels;        // the box's shape, x fastest
	const uint32_t *colors;        // entry L - 1: A in bits 24 .. 31; null: every non-zero label is visible
	uint32_t        entries;       // min(table_entries, 2^32 - 1)
	int             bw, bh;        // the labels' row and slice: the box's width and height
};

// What a lane holds of one row of labels: x .. x + 3 (zero past the row's end) and x + 4, the first label of the lane above (wave_shl:1;
// every lane of the wave takes part), in the wave's last lane a dword load.  WIDE (bw >= 4): one 16-byte load at min(x, bw - 4), at any
// 4-byte alignment, shifted down where it was moved; narrower rows gather.  Nothing outside the row is read; what is not a label of the row
// only reaches cubes that are not counted.
struct Lab5
{
	uint32_t v[5];
};

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

template <bool WIDE>
__device__ __forceinline__ Lab5 lab5(const uint32_t *row, int x, int bw, uint32_t lane)
{
	Lab5 r;
	if (WIDE)
	{
		const u32x4_a4 q = *reinterpret_cast<const u32x4_a4 *>(row + min(x, bw - 4));
		r.v[0] = q.x, r.v[1] = q.y, r.v[2] = q.z, r.v[3] = q.w;
		const int over = x + 4 - bw;
#pragma unroll
		for (int s = 1; s <= 4; ++s)
			if (over >= s)
				r.v[0] = r.v[1], r.v[1] = r.v[2], r.v[2] = r.v[3], r.v[3] = 0u;
	}
	else
	{
#pragma unroll
		for (int i = 0; i < 4; ++i)
			r.v[i] = x + i < bw ? row[x + i] : 0u;
	}
	r.v[4] = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) r.v[0], 0x130, 0xf, 0xf, false);        // wave_shl:1
	if (lane == 63)
		r.v[4] = row[min(x + 4, bw - 1)];
	return r;
}

// the rows of a cube's corners: slice * 2 + row, so that corner j of the lane's cube i is label i + (j & 1) of row j >> 1
struct CubeRows
{
	Lab5 r[4];
};

// the eight labels with the hidden ones replaced by 0.  The table is read once per distinct label, at the label's first corner, and every
// read is issued before the first word is looked at
__device__ __forceinline__ void shown8(const LabelGeom &A, const uint32_t c[8], uint32_t E[8])
{
	if (!A.colors)
	{
#pragma unroll
		for (int j = 0; j < 8; ++j)
			E[j] = c[j];
		return;
	}
	uint32_t word[8];
#pragma unroll
	for (int j = 0; j < 8; ++j)
	{
		bool first = c[j] - 1u < A.entries;        // label 0 gives 2^32 - 1, which no table names
#pragma unroll
		for (int k = 0; k < j; ++k)
			first = first && c[k] != c[j];
		word[j] = 0u;
		if (first)
			word[j] = A.colors[c[j] - 1u];
	}
#pragma unroll
	for (int j = 0; j < 8; ++j)
	{
		uint32_t w = word[j];        // the word of the label's first corner: the others hold 0
#pragma unroll
		for (int k = 0; k < j; ++k)
			w |= c[k] == c[j] ? word[k] : 0u;
		E[j] = (w >> 24) != 0u ? c[j] : 0u;
	}
}

// the triangles of a group of pc local vertices
__device__ __forceinline__ uint32_t group_triangles(uint32_t pc) { return pc == 2u ? 2u : pc == 4u ? 0u : 1u; }

// the triangles of a tetrahedron with the (shown) labels l0 .. l3 at its local vertices
__device__ __forceinline__ uint32_t tet_count(uint32_t l0, uint32_t l1, uint32_t l2, uint32_t l3)
{
	uint32_t n = 0;
	if (l0 != 0u)
		n += group_triangles(1u + (l1 == l0) + (l2 == l0) + (l3 == l0));
	if (l1 != 0u && l1 != l0)
		n += group_triangles(1u + (l2 == l1) + (l3 == l1));
	if (l2 != 0u && l2 != l0 && l2 != l1)
		n += group_triangles(1u + (l3 == l2));
	if (l3 != 0u && l3 != l0 && l3 != l1 && l3 != l2)
		n += 1u;
	return n;
}

// the triangles of the cube with the shown labels E; lut: mtet_table.hpp's count by corner mask
__device__ __forceinline__ uint32_t shown_cube_count(const uint8_t *lut, const uint32_t E[8])
{
	uint32_t top = 0;
#pragma unroll
	for (int j = 0; j < 8; ++j)
		top = max(top, E[j]);
	if (top == 0u)
		return 0u;
	uint32_t cm  = 0;
	bool     one = true;
#pragma unroll
	for (int j = 0; j < 8; ++j)
	{
		cm |= (E[j] != 0u ? 1u : 0u) << j;
		one = one && (E[j] == 0u || E[j] == top);
	}
	if (one)        // one visible label: the isosurface's cube
		return lut[cm];
	uint32_t n = 0;
#pragma unroll
	for (int t = 0; t < 6; ++t)
		n += tet_count(E[0], E[kMtetCorners[t][1]], E[kMtetCorners[t][2]], E[7]);
	return n;
}

// the triangles of the cube with the labels c
__device__ __forceinline__ uint32_t cube_count(const LabelGeom &A, const uint8_t *lut, const uint32_t c[8])
{
	uint32_t dif = 0;
#pragma unroll
	for (int j = 1; j < 8; ++j)
		dif |= c[j] ^ c[0];
	if (dif == 0u)
		return 0u;
	uint32_t E[8];
	shown8(A, c, E);
	return shown_cube_count(lut, E);
}

// the triangles of the lane's first nvalid cubes
__device__ __forceinline__ uint32_t lane_count(const LabelGeom &A, const uint8_t *lut, const CubeRows &R, int nvalid)
{
	uint32_t dif = 0;
#pragma unroll
	for (int j = 0; j < 4; ++j)
#pragma unroll
		for (int i = 0; i < 5; ++i)
			dif |= R.r[j].v[i] ^ R.r[0].v[0];
	if (dif == 0u)
		return 0u;
	uint32_t n = 0;
#pragma unroll
	for (int i = 0; i < 4; ++i)
		if (i < nvalid)
		{
			uint32_t c[8];
#pragma unroll
			for (int j = 0; j < 8; ++j)
				c[j] = R.r[j >> 1].v[i + (j & 1)];
			n += cube_count(A, lut, c);
		}
	return n;
}

__device__ __forceinline__ uint32_t sel4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, int i) { return i == 0 ? a : i == 1 ? b : i == 2 ? c : d; }

// the labels of the lane's cube i, corner j in c[j]; i need not be known at compile time
__device__ __forceinline__ void cube_labels(const CubeRows &R, int i, uint32_t c[8])
{
#pragma unroll
	for (int j = 0; j < 8; ++j)
	{
		const Lab5 &r = R.r[j >> 1];
		c[j]          = (j & 1) ? sel4(r.v[1], r.v[2], r.v[3], r.v[4], i) : sel4(r.v[0], r.v[1], r.v[2], r.v[3], i);
	}
}

// the five voxels x .. x + 4 of a row of the volume as one 64-bit value (zero past the row's end): a dword at any alignment and, as in lab5(),
// the first byte of the lane above (every lane of the wave takes part), in the wave's last lane a byte load.  Nothing outside the row is read
__device__ __forceinline__ uint64_t bytes5(const uint8_t *row, int x, int W, uint32_t lane)
{
	const uint32_t d = x < W ? load4_clipped(row, x, W) : 0u;
	uint32_t       e = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) d, 0x130, 0xf, 0xf, false) & 0xffu;        // wave_shl:1
	if (lane == 63)
		e = row[min(x + 4, W - 1)];
	return (uint64_t) d | (uint64_t) e << 32;
}

// the lane's cube i of four bytes5() rows (slice * 2 + row), corner j in byte j: bytes i and i + 1 of row j >> 1
__device__ __forceinline__ uint64_t cube_bytes(const CubeBytes &B, int i)
{
	uint64_t cb = 0;
#pragma unroll
	for (int r = 0; r < 4; ++r)
		cb |= ((B.v[r] >> (8 * i)) & 0xffffull) << (16 * r);
	return cb;
}

// where the vertex lies on the edge from corner a to corner b of a cube: halfway unless the volume (cb: the cube's eight bytes, corner j in
// byte j; read with a volume only) crosses iso between them
__device__ __forceinline__ float label_edge_t(bool with_volume, uint64_t cb, uint32_t a, uint32_t b, float iso)
{
	float t = 0.5f;
	if (with_volume)
	{
		const float fa = (float) ((uint32_t) (cb >> (8u * a)) & 0xffu) * kInv255, fb = (float) ((uint32_t) (cb >> (8u * b)) & 0xffu) * kInv255;
		if ((fa >= iso) != (fb >= iso))
			t = (iso - fa) / (fb - fa);
	}
	return t;
}

// the vertex on the edge `code` = a | b << 3 of the cube with origin (cx, cy, cz) in the volume: from a towards b by t
__device__ __forceinline__ void label_edge_vertex(float t, uint32_t code, int cx, int cy, int cz, float *out)
{
	const uint32_t a = code & 7u, dif = a ^ (code >> 3);
	const float    ax = (float) (cx + (int) (a & 1u)), ay = (float) (cy + (int) ((a >> 1) & 1u)), az = (float) (cz + (int) (a >> 2));
	out[0] = (dif & 1u) ? ax + t : ax;
	out[1] = (dif & 2u) ? ay + t : ay;
	out[2] = (dif & 4u) ? az + t : az;
}

// the same from the edge alone: a = the voxel of the lower local index, never the label
__device__ __forceinline__ void label_edge_vertex(bool with_volume, uint64_t cb, uint32_t code, int cx, int cy, int cz, float iso, float *out)
{
	label_edge_vertex(label_edge_t(with_volume, cb, code & 7u, code >> 3, iso), code, cx, cy, cz, out);
}

// ---- host side
// the kernels' argument block of a call over box b with the plan p; d_vol null: the volume is not read
inline LabelGeom label_geom(const uint32_t *d_labels, VkvExtent3D e, const VkvBox &b, const uint32_t *d_colors, uint64_t table_entries, const uint8_t *d_vol,
                            const uint8_t *d_visibility_map, VkvExtent3D me, const MeshPlan &p)
{
	LabelGeom A{};
	A.G     = mesh_geom(d_vol, e, b, 0.0f, d_visibility_map, me, p);
	A.G.thr = 1u;        // of the visibility map's bytes, 255 passes and 0 does not
	A.labels = d_labels, A.colors = d_colors, A.entries = table_entries > 0xffffffffull ? 0xffffffffu : (uint32_t) table_entries;
	A.bw = (int) b.width, A.bh = (int) b.height;
	return A;
}

}        // namespace vkv
