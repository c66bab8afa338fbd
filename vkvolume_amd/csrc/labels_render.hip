// labels_render.hip — a label volume as a picture (vkv_render_labels) and its skipping map (vkv_label_visibility_map).  DESIGN.md §5.21 pins
// every output to the bit and says why skipping over the visibility map gives the dense path's bits.
//
// Labels: a uint32 array of the shape of a box of the volume (the output of vkv_label_components, vkv_propagate_labels,
// vkv_geodesic_propagate), read with nearest-voxel addressing: the voxel of a texture-space point is floor(c + 0.5) of the samplers' own
// coordinate c = fma(q, extent, -0.5), clamped to the volume; a voxel outside the box carries label 0.  A label L is visible when the colour
// table names it (1 <= L <= table_entries) and the alpha byte of its entry L - 1 is not 0.
//
// Visibility map: one byte per cell of the max map's geometry, 255 where a voxel of the cell grown by one voxel per side carries a visible
// label, else 0.  One lane per cell; a label of 0 (most voxels) needs no table lookup.
//
// Render: rays, workgroup deal, wave patch shape, depth and stores are the direct renderers' (direct_render.hpp).  The dense variant loads
// kDenseGroup labels per round, then looks their colours up, and stops after the round that holds the first visible sample; the skipping
// variant probes the visibility map once per cell entered (max_map_skip<true> with bound 1: a byte of 0 is skipped, one of 255 never).  A
// hit lane then spends refine_steps label lookups on the bisection and, with shade == 1, four filtered samples of the volume on the
// tetrahedron gradient (k_iso's shading, restated here: iso.hip stays as it is).
#include <cmath>

#include "ray_setup.hpp"
#include "volume_sampling.hpp"
#include "direct_render.hpp"
#include "box_domain.hpp"

namespace
{

// the labels, their box and the colour table as the kernels read them
struct LabelTable
{
	const uint32_t *labels;        // the box's shape, x fastest
	const uint32_t *colors;        // entry L - 1: R | G << 8 | B << 16 | A << 24
	uint32_t        entries;       // min(table_entries, 2^32 - 1): label 0 gives L - 1 = 2^32 - 1, which no table names
	int             x0, y0, z0;    // the box's first voxel
	uint32_t        bw, bh, bd;    // the box's shape
};

// the label of the volume's voxel (x, y, z); 0 outside the box
__device__ __forceinline__ uint32_t label_of_voxel(const LabelTable &T, int x, int y, int z)
{
	const uint32_t ux = (uint32_t) (x - T.x0), uy = (uint32_t) (y - T.y0), uz = (uint32_t) (z - T.z0);
	if (ux >= T.bw || uy >= T.bh || uz >= T.bd)
		return 0u;
	return T.labels[((size_t) uz * (size_t) T.bh + (size_t) uy) * (size_t) T.bw + (size_t) ux];
}

// the colour word of label L; 0 (alpha 0: not visible) for label 0 and for a label the table does not name
__device__ __forceinline__ uint32_t color_of_label(const LabelTable &T, uint32_t L)
{
	const uint32_t e = L - 1u;
	return e < T.entries ? T.colors[e] : 0u;
}

__device__ __forceinline__ bool word_visible(uint32_t c) { return (c >> 24) != 0u; }

// ---- the visibility map -----------------------------------------------------------------------------------------------------------------

struct VisibilityMapArgs
{
	LabelTable T;
	uint8_t *  map;
	int        W, H, D, mw, mh, md, bx, by, bz;
};

__global__ void __launch_bounds__(256) k_label_visibility_map(const VisibilityMapArgs a)
{
	const uint64_t t = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (t >= (uint64_t) a.mw * (uint64_t) a.mh * (uint64_t) a.md)
		return;
	const int      cx = (int) (t % (uint64_t) a.mw);
	const uint64_t r  = t / (uint64_t) a.mw;
	const int      cy = (int) (r % (uint64_t) a.mh), cz = (int) (r / (uint64_t) a.mh);
	const LabelTable &T = a.T;
	bool              seen = false;
	if (cx * a.bx < a.W && cy * a.by < a.H && cz * a.bz < a.D)        // (cells past the volume hold 0)
	{
		// the cell's voxel box grown by one voxel, clipped to the volume and to the labels' box (inclusive; empty where lo > hi)
		const int x0 = max(max(cx * a.bx - 1, 0), T.x0), x1 = min(min(cx * a.bx + a.bx, a.W - 1), T.x0 + (int) T.bw - 1);
		const int y0 = max(max(cy * a.by - 1, 0), T.y0), y1 = min(min(cy * a.by + a.by, a.H - 1), T.y0 + (int) T.bh - 1);
		const int z0 = max(max(cz * a.bz - 1, 0), T.z0), z1 = min(min(cz * a.bz + a.bz, a.D - 1), T.z0 + (int) T.bd - 1);
		for (int z = z0; z <= z1 && !seen; ++z)
		{
			// a slice of the box at a time: first every label ORed together, with no branch between the loads (most slices hold only label
			// 0 and end here); the table is looked up, label by label, only in a slice that holds a label at all
			const uint32_t *slice = T.labels + (size_t) (z - T.z0) * (size_t) T.bh * (size_t) T.bw;
			uint32_t        any   = 0u;
			for (int y = y0; y <= y1; ++y)
			{
				const uint32_t *row = slice + (size_t) (y - T.y0) * (size_t) T.bw;
				for (int x = x0; x <= x1; ++x)
					any |= row[x - T.x0];
			}
			if (any == 0u)
				continue;
			for (int y = y0; y <= y1; ++y)
			{
				const uint32_t *row = slice + (size_t) (y - T.y0) * (size_t) T.bw;
				for (int x = x0; x <= x1; ++x)
				{
					const uint32_t L = row[x - T.x0];
					if (L != 0u && word_visible(color_of_label(T, L)))
						seen = true;
				}
			}
		}
	}
	a.map[t] = seen ? (uint8_t) 255 : (uint8_t) 0;
}

// ---- the render --------------------------------------------------------------------------------------------------------------------------

struct LabelRenderArgs
{
	RayMarchArgs   A;               // the fields ray_setup, start_entry and the samplers read (fill_direct_args)
	LabelTable     T;
	int            refine_steps;    // 0 .. 16
	float          ambient, diffuse, specular;
	uint32_t       shininess;       // 1 .. 1024
	uint32_t *     out_label;       // or null
	float *        out_normal;      // or null
	MaxMapGeometry mm;              // skipping variant only: the visibility map
};

// the voxel of a texture-space coordinate on one axis: floor(c + 0.5) of the samplers' coordinate c, clamped
__device__ __forceinline__ int voxel_of(float q, int extent)
{
	const float c = __builtin_fmaf(q, (float) extent, -0.5f);
	return i_clamp((int) __builtin_floorf(c + 0.5f), 0, extent - 1);
}

__device__ __forceinline__ uint32_t label_at(const RayMarchArgs &A, const LabelTable &T, float qx, float qy, float qz)
{
	return label_of_voxel(T, voxel_of(qx, A.W), voxel_of(qy, A.H), voxel_of(qz, A.D));
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz)
{
	return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
}

// k_iso's normal and headlight at the hit point h of a ray with step (R.sx, R.sy, R.sz), in its order of operations: the unit normal facing
// the camera into n, the light term L as the result
template <bool PACKED>
__device__ __forceinline__ float headlight(const LabelRenderArgs &I, const Ray &R, float hx, float hy, float hz, float &nx, float &ny, float &nz)
{
	const RayMarchArgs &A = I.A;
	// gradient: the integrator's tetrahedron taps, in texture space
	const float dix = 1.0f / (float) A.W, diy = 1.0f / (float) A.H, diz = 1.0f / (float) A.D;
	const float t1  = mip_sample<PACKED>(A, hx + dix, hy - diy, hz - diz);
	const float t2  = mip_sample<PACKED>(A, hx - dix, hy - diy, hz + diz);
	const float t3  = mip_sample<PACKED>(A, hx - dix, hy + diy, hz - diz);
	const float t4  = mip_sample<PACKED>(A, hx + dix, hy + diy, hz + diz);
	const float gx  = (((t1 - t2) - t3) + t4) * 0.25f;
	const float gy  = (((-t1 - t2) + t3) + t4) * 0.25f;
	const float gz  = (((-t1 + t2) - t3) + t4) * 0.25f;
	const float gtx = gx * (float) A.W, gty = gy * (float) A.H, gtz = gz * (float) A.D;
	// world-space normal: transpose(model_inv[3x3]) * g_tex
	const float *mi = A.model_inv;
	const float  wx = dot3(mi[0], mi[1], mi[2], gtx, gty, gtz), wy = dot3(mi[4], mi[5], mi[6], gtx, gty, gtz), wz = dot3(mi[8], mi[9], mi[10], gtx, gty, gtz);
	// view vector: -(model[3x3] * step), normalised
	const float *m  = A.model;
	float        vx = -dot3(m[0], m[4], m[8], R.sx, R.sy, R.sz), vy = -dot3(m[1], m[5], m[9], R.sx, R.sy, R.sz), vz = -dot3(m[2], m[6], m[10], R.sx, R.sy, R.sz);
	const float  vl = __builtin_sqrtf(dot3(vx, vy, vz, vx, vy, vz));
	vx = vx / vl, vy = vy / vl, vz = vz / vl;
	const float l2 = dot3(wx, wy, wz, wx, wy, wz);
	if (l2 == 0.0f || !__builtin_isfinite(l2))
		nx = vx, ny = vy, nz = vz;
	else
	{
		const float nl = __builtin_sqrtf(l2);
		nx = wx / nl, ny = wy / nl, nz = wz / nl;
		if (dot3(nx, ny, nz, vx, vy, vz) < 0.0f)
			nx = -nx, ny = -ny, nz = -nz;        // two-sided: the normal faces the camera
	}
	// the half vector is v; spec = d^shininess by binary exponentiation, highest bit first
	const float d = g_clamp(dot3(nx, ny, nz, vx, vy, vz), 0.0f, 1.0f);
	float       r = 1.0f;
	for (int bit = 10; bit >= 0; --bit)
	{
		r = r * r;
		if ((I.shininess >> bit) & 1u)
			r = r * d;
	}
	return (I.ambient + I.diffuse * d) + I.specular * r;
}

// SHADE: 0 flat colours (the volume is not read), 1 lit from the linear volume, 2 lit from the packed image
template <int SHADE, bool SKIP>
__global__ void __launch_bounds__(256) k_labels(const LabelRenderArgs I)
{
	const RayMarchArgs &A = I.A;
	const LabelTable &  T = I.T;
	uint32_t            px, py, o;
	if (!pixel_deal(A, A.wave_pw_log2, px, py, o))
		return;
	Ray R;
	R.o                = o;
	const bool marched = ray_setup<VKV_SKIP_NONE>(A, px, py, R);
	int        k       = -1;        // the first index of a sample with a visible label
	uint32_t   n_look = 0, n_probe = 0, n_skip = 0;
	if (!SKIP && marched)
	{
		// dense: kDenseGroup labels per round, every label load issued before the first colour lookup; the round that holds the first hit
		// ends the march (its samples past the hit are not counted)
		const int n = R.n_steps;
		int       i = 0;
		for (; i + kDenseGroup <= n; i += kDenseGroup)
		{
			uint32_t L[kDenseGroup], c[kDenseGroup];
#pragma unroll
			for (int j = 0; j < kDenseGroup; ++j)
			{
				const float fi = (float) (i + j);
				L[j] = label_at(A, T, __builtin_fmaf(fi, R.sx, R.ex), __builtin_fmaf(fi, R.sy, R.ey), __builtin_fmaf(fi, R.sz, R.ez));
			}
#pragma unroll
			for (int j = 0; j < kDenseGroup; ++j)
				c[j] = color_of_label(T, L[j]);
			int hit = -1;
#pragma unroll
			for (int j = kDenseGroup - 1; j >= 0; --j)
				if (word_visible(c[j]))
					hit = j;
			if (hit >= 0)
			{
				k = i + hit;
				break;
			}
		}
		if (k < 0)
			for (; i < n; ++i)
			{
				const float fi = (float) i;
				if (word_visible(color_of_label(T, label_at(A, T, __builtin_fmaf(fi, R.sx, R.ex), __builtin_fmaf(fi, R.sy, R.ey), __builtin_fmaf(fi, R.sz, R.ez)))))
				{
					k = i;
					break;
				}
			}
		n_look = k >= 0 ? (uint32_t) (k + 1) : (uint32_t) n;
	}
	if (SKIP && marched)
	{
		const int n         = R.n_steps;
		uint32_t  last_cell = ~0u;
		int       i         = 0;
		while (i < n)
		{
			const float fi   = (float) i;
			const float posx = __builtin_fmaf(fi, R.sx, R.ex), posy = __builtin_fmaf(fi, R.sy, R.ey), posz = __builtin_fmaf(fi, R.sz, R.ez);
			// a cell without a visible voxel (byte 0: 0 * kInv255 < 1; a byte of 255 gives 255 * kInv255 == 1): jump over its samples
			const int last = max_map_skip<true>(A, I.mm, R, i, n, posx, posy, posz, 1.0f, last_cell, n_probe);
			if (last >= 0)
			{
				n_skip += (uint32_t) (last + 1 - i);
				i = last + 1;
				continue;
			}
			++n_look;
			if (word_visible(color_of_label(T, label_at(A, T, posx, posy, posz))))
			{
				k = i;
				break;
			}
			++i;
		}
	}
	const size_t po = o;
	float        cr = 0.0f, cg = 0.0f, cb = 0.0f, ca = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f, nw = 0.0f;
	uint32_t     hit_label = 0u;
	float        depth     = A.depth_attachment ? A.in_depth[po] : 0.0f;        // what the integrator gives a pixel without colour
	if (k >= 0)
	{
		// refinement: bisection between samples k - 1 and k on the predicate "the label here is visible" (t = 0 for a hit at the first sample)
		float th = 0.0f;
		if (k > 0)
		{
			float lo = (float) (k - 1);
			th       = (float) k;
			for (int j = 0; j < I.refine_steps; ++j)
			{
				const float mid = (lo + th) * 0.5f;
				if (word_visible(color_of_label(T, label_at(A, T, __builtin_fmaf(mid, R.sx, R.ex), __builtin_fmaf(mid, R.sy, R.ey), __builtin_fmaf(mid, R.sz, R.ez)))))
					th = mid;
				else
					lo = mid;
			}
		}
		const float hx = __builtin_fmaf(th, R.sx, R.ex), hy = __builtin_fmaf(th, R.sy, R.ey), hz = __builtin_fmaf(th, R.sz, R.ez);
		hit_label       = label_at(A, T, hx, hy, hz);        // visible: th only ever sits where the predicate held
		const uint32_t c = color_of_label(T, hit_label);
		if (A.out_depth)
			depth = first_hit_depth(A, hx, hy, hz);
		cr = (float) (c & 255u) * kInv255, cg = (float) ((c >> 8) & 255u) * kInv255, cb = (float) ((c >> 16) & 255u) * kInv255, ca = 1.0f;
		if (SHADE != 0)
		{
			const float L = headlight<SHADE == 2>(I, R, hx, hy, hz, nx, ny, nz);
			nw = 1.0f;
			cr = g_clamp(cr * L, 0.0f, 1.0f), cg = g_clamp(cg * L, 0.0f, 1.0f), cb = g_clamp(cb * L, 0.0f, 1.0f);
		}
	}
	if (A.out_color)
		store_float4_nt(A.out_color, po, cr, cg, cb, ca);
	if (A.out_rgba8)
		store_rgba8_nt(A.out_rgba8, po, cr, cg, cb, ca);
	if (I.out_label)
		__builtin_nontemporal_store(hit_label, I.out_label + po);
	if (I.out_normal)
		store_float4_nt(I.out_normal, po, nx, ny, nz, nw);
	if (A.out_counts)
		store_counts(A.out_counts, po, n_look, n_probe, n_skip);
	if (A.out_depth)
		__builtin_nontemporal_store(depth, A.out_depth + po);
}

bool finite_nonneg(float x) { return std::isfinite(x) && x >= 0.0f; }

// what both entry points check of the labels, their box and the table (`what`: the entry point's name in the messages); VKV_OK or the code
int check_label_table(vkv_ctx *ctx, const char *what, const uint32_t *d_labels, VkvExtent3D extent, const VkvBox *box, const uint32_t *d_colors,
                      uint64_t table_entries)
{
	if (!d_labels)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: null d_labels", what);
	if (!d_colors && table_entries != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: a table of %llu entries needs d_colors", what, (unsigned long long) table_entries);
	if ((((uintptr_t) d_labels | (uintptr_t) d_colors) & 3u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: d_labels and d_colors must be 4-byte aligned", what);
	if (const int rc = check_box(ctx, what, extent, box))
		return rc;
	if (!components_launch_ok(extent, box))
		return set_error(ctx, VKV_E_UNSUPPORTED, "%s: a box of more than 2^32 - 1 voxels", what);
	return VKV_OK;
}

LabelTable label_table(const uint32_t *d_labels, VkvExtent3D extent, const VkvBox *box, const uint32_t *d_colors, uint64_t table_entries)
{
	const VkvBox b = whole_or(extent, box);
	LabelTable   t;
	t.labels = d_labels, t.colors = d_colors, t.entries = table_entries > 0xffffffffull ? 0xffffffffu : (uint32_t) table_entries;
	t.x0 = (int) b.x0, t.y0 = (int) b.y0, t.z0 = (int) b.z0, t.bw = b.width, t.bh = b.height, t.bd = b.depth;
	return t;
}

// the checks of vkv_render_labels; VKV_OK or the code (nothing is enqueued before they pass)
int check_labels(vkv_ctx *ctx, const VkvRenderParams *P, const VkvLabelRenderOptions *O)
{
	if (!P || !O)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_labels: null params or options");
	if (O->flags != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_labels: flags must be 0");
	if (O->shade > 1)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_labels: shade must be 0 or 1");
	if (O->refine_steps > 16)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_labels: refine_steps must be 0 .. 16");
	if (!finite_nonneg(O->ambient) || !finite_nonneg(O->diffuse) || !finite_nonneg(O->specular))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_labels: ambient, diffuse and specular must be finite and >= 0");
	if (O->shininess < 1 || O->shininess > 1024)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_labels: shininess must be 1 .. 1024");
	// shade == 0 reads no voxel: the volume may be null
	if (const int rc = check_first_hit_params(ctx, "render_labels", P, O->d_visibility_map, O->d_out_label != nullptr || O->d_out_normal != nullptr, true,
	                                          O->shade != 0))
		return rc;
	return check_label_table(ctx, "render_labels", O->d_labels, P->volume_extent, O->box, O->d_colors, O->table_entries);
}

template <int SHADE>
void launch_labels(const LabelRenderArgs &a, hipStream_t s)
{
	if (a.mm.max_map)
		hipLaunchKernelGGL((k_labels<SHADE, true>), dim3(deal_grid(a.A)), dim3(256), 0, s, a);
	else
		hipLaunchKernelGGL((k_labels<SHADE, false>), dim3(deal_grid(a.A)), dim3(256), 0, s, a);
}

}        // namespace

extern "C" {

int vkv_label_visibility_map(vkv_ctx *ctx, const uint32_t *d_labels, VkvExtent3D extent, const VkvBox *box, const uint32_t *d_colors,
                             uint64_t table_entries, VkvExtent3D map_extent, uint8_t *d_map, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_map || !extent_ok(extent) || !map_extent_ok(extent, map_extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "label_visibility_map: null d_map or bad extent");
	if (const int rc = check_label_table(ctx, "label_visibility_map", d_labels, extent, box, d_colors, table_entries))
		return rc;
	const uint64_t cells  = (uint64_t) map_extent.width * map_extent.height * map_extent.depth;
	const uint64_t groups = (cells + 255) / 256;
	if (groups > 0x7fffffffull)
		return set_error(ctx, VKV_E_UNSUPPORTED, "label_visibility_map: map too large for one launch");
	VisibilityMapArgs a;
	a.T   = label_table(d_labels, extent, box, d_colors, table_entries);
	a.map = d_map;
	a.W = (int) extent.width, a.H = (int) extent.height, a.D = (int) extent.depth;
	a.mw = (int) map_extent.width, a.mh = (int) map_extent.height, a.md = (int) map_extent.depth;
	a.bx = (int) block_of(extent.width, map_extent.width), a.by = (int) block_of(extent.height, map_extent.height), a.bz = (int) block_of(extent.depth, map_extent.depth);
	hipLaunchKernelGGL(k_label_visibility_map, dim3((uint32_t) groups), dim3(256), 0, (hipStream_t) stream, a);
	return check_launch(ctx, "label_visibility_map");
}

int vkv_render_labels(vkv_ctx *ctx, const VkvRenderParams *P, const VkvLabelRenderOptions *O, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	const int rc = check_labels(ctx, P, O);
	if (rc != VKV_OK)
		return rc;
	LabelRenderArgs a;
	fill_direct_args(P, a.A);
	if (a.A.nblocks == 0)
		return VKV_OK;
	a.T            = label_table(O->d_labels, P->volume_extent, O->box, O->d_colors, O->table_entries);
	a.refine_steps = (int) O->refine_steps, a.shininess = O->shininess;
	a.ambient = O->ambient, a.diffuse = O->diffuse, a.specular = O->specular;
	a.out_label = O->d_out_label, a.out_normal = O->d_out_normal;
	fill_max_map_geometry(P, O->d_visibility_map, a.mm);
	if (O->shade == 0)
		launch_labels<0>(a, (hipStream_t) stream);
	else if (a.A.packed)
		launch_labels<2>(a, (hipStream_t) stream);
	else
		launch_labels<1>(a, (hipStream_t) stream);
	return check_launch(ctx, "render_labels");
}

}        // extern "C"
