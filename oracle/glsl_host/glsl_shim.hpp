// The part of GLSL 4.60 that the reference's compute shaders and its fragment shader use, as plain C++17: vector types with the swizzles those
// shaders read and write, mixed int / float vector arithmetic, the builtins, and images / samplers over raw uint8 arrays ([D][H][W], x fastest).
// Own code: it holds no shader text.  oracle/glsl_host/prep.py turns a shader file into a C++ source (under oracle/_ref/ only) that includes
// this header; oracle/glsl_host/harness.cpp sets the resources and loops over invocations.  Test infrastructure only.
//
// Everything the Vulkan implementation is free to choose lives HERE, as the pins of DESIGN.md section 3, never in the shader text:
//   R8_UNORM load = byte / 255; R8_UNORM store = rint(clamp(v, 0, 1) * 255); the clamp-to-edge linear filter; the NEAREST lookup of the
//   transfer-function texture; the forms of length / normalize / distance; min() of a NaN (0 * inf on an axis-parallel ray); the association
//   of `proj * view * model * v`.
// Two arithmetic modes (glsl::g_pinned):
//   0 "plain"   every a + b * c is a multiply followed by an add; the filter is the Vulkan specification's weighted sum over eight texels;
//               normalize(v) = v / sqrt((x*x + y*y) + z*z); min / max exactly as the GLSL specification writes them.  (What
//               tests/golden/frag_literal.py calls "plain".)
//   1 "pinned"  the contractions that DESIGN.md section 3 pins: a `float * vec` (or `vec * float`, `vec * int`) product is LAZY and an addition
//               that consumes it is one fma per component (this is `ray_entry + float(i) * step_volume`, `tFar * dir + front`, the blend
//               `out_color + (1 - a) * color` and `ray_entry + step_volume * i_first_hit`; on every other such pair in the shaders one
//               factor is +-1, 0 or an integer below 256 times +-1, so the product is exact and the fma changes nothing); the fma filter on
//               the bytes; the fma forms of normalize / distance; mat4 * vec4 as an fma chain; min() ignores a NaN operand.
// Statement-level arithmetic in the shader text is compiled with -ffp-contract=off: nothing is fused that is not written as fmaf here.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace glsl
{
typedef unsigned int uint;

inline int g_pinned = 1;

struct vec3;
struct ivec3;
struct uvec3;
struct vec4;

// ---- swizzle proxies: members of a union that aliases the components ----------------------------------------------------------------
template <class V, class T, int N, int A, int B, int C>
struct swz3
{
	T d[N];
	operator V() const { return V(d[A], d[B], d[C]); }
	swz3 &operator=(const V &v)
	{
		const T a = v.x, b = v.y, c = v.z;
		d[A] = a, d[B] = b, d[C] = c;
		return *this;
	}
	swz3 &operator*=(T s)
	{
		d[A] *= s, d[B] *= s, d[C] *= s;
		return *this;
	}
};

struct vec2
{
	float x, y;
	vec2() : x(0), y(0) {}
	vec2(float a, float b) : x(a), y(b) {}
};

struct vec3
{
	union
	{
		struct { float x, y, z; };
		struct { float r, g, b; };
		swz3<vec3, float, 3, 0, 1, 2> xyz;
	};
	vec3() : x(0), y(0), z(0) {}
	explicit vec3(float s) : x(s), y(s), z(s) {}
	vec3(float a, float b, float c) : x(a), y(b), z(c) {}
	vec3(const vec3 &o) : x(o.x), y(o.y), z(o.z) {}
	vec3 &operator=(const vec3 &o) { x = o.x, y = o.y, z = o.z; return *this; }
	explicit vec3(const ivec3 &v);
	explicit vec3(const vec4 &v);
	explicit operator uint() const { return (uint) x; } // a scalar constructed from a vector takes its first component
};

struct ivec2
{
	union
	{
		struct { int x, y; };
		swz3<ivec3, int, 2, 0, 1, 1> xyy;
		swz3<ivec3, int, 2, 1, 1, 0> yyx;
		swz3<ivec3, int, 2, 1, 0, 1> yxy;
		swz3<ivec3, int, 2, 0, 0, 0> xxx;
	};
	ivec2() : x(0), y(0) {}
	ivec2(int a, int b) : x(a), y(b) {}
};

struct ivec3
{
	union
	{
		struct { int x, y, z; };
		swz3<ivec3, int, 3, 0, 1, 2> xyz;
	};
	ivec3() : x(0), y(0), z(0) {}
	explicit ivec3(int s) : x(s), y(s), z(s) {}
	ivec3(int a, int b, int c) : x(a), y(b), z(c) {}
	ivec3(const ivec3 &o) : x(o.x), y(o.y), z(o.z) {}
	ivec3 &operator=(const ivec3 &o) { x = o.x, y = o.y, z = o.z; return *this; }
	explicit ivec3(const vec3 &v) : x((int) v.x), y((int) v.y), z((int) v.z) {} // truncates toward zero
	explicit ivec3(const uvec3 &v);
};

struct uvec3
{
	uint x, y, z;
	uvec3() : x(0), y(0), z(0) {}
	uvec3(uint a, uint b, uint c) : x(a), y(b), z(c) {}
};

struct ivec4
{
	union
	{
		struct { int x, y, z, w; };
		swz3<ivec3, int, 4, 0, 1, 2> xyz;
	};
	ivec4() : x(0), y(0), z(0), w(0) {}
	explicit ivec4(int s) : x(s), y(s), z(s), w(s) {}
	ivec4(int a, int b, int c, int d) : x(a), y(b), z(c), w(d) {}
	ivec4(const ivec4 &o) : x(o.x), y(o.y), z(o.z), w(o.w) {}
	ivec4 &operator=(const ivec4 &o) { x = o.x, y = o.y, z = o.z, w = o.w; return *this; }
};

struct uvec4
{
	uint x, y, z, w;
	uvec4() : x(0), y(0), z(0), w(0) {}
	explicit uvec4(uint s) : x(s), y(s), z(s), w(s) {}
	uvec4(uint a, uint b, uint c, uint d) : x(a), y(b), z(c), w(d) {}
};

struct bvec3
{
	bool x, y, z;
	bvec3(bool a, bool b, bool c) : x(a), y(b), z(c) {}
};

struct vec4
{
	union
	{
		struct { float x, y, z, w; };
		struct { float r, g, b, a; };
		swz3<vec3, float, 4, 0, 1, 2> xyz;
		swz3<vec3, float, 4, 0, 1, 2> rgb;
	};
	vec4() : x(0), y(0), z(0), w(0) {}
	explicit vec4(float s) : x(s), y(s), z(s), w(s) {}
	vec4(float a, float b, float c, float d) : x(a), y(b), z(c), w(d) {}
	vec4(const vec3 &v, float d) : x(v.x), y(v.y), z(v.z), w(d) {}
	vec4(const vec4 &o) : x(o.x), y(o.y), z(o.z), w(o.w) {}
	vec4 &operator=(const vec4 &o) { x = o.x, y = o.y, z = o.z, w = o.w; return *this; }
	vec4 &operator/=(float s) // by value: `v /= v.w` divides every component, w last, by the w it had
	{
		x /= s, y /= s, z /= s, w /= s;
		return *this;
	}
};

inline vec3::vec3(const ivec3 &v) : x((float) v.x), y((float) v.y), z((float) v.z) {}
inline vec3::vec3(const vec4 &v) : x(v.x), y(v.y), z(v.z) {}
inline ivec3::ivec3(const uvec3 &v) : x((int) v.x), y((int) v.y), z((int) v.z) {}

// ---- lazy scalar * vector products (see "pinned" above) -------------------------------------------------------------------------------
struct lazy3
{
	float s;
	vec3  v;
	operator vec3() const { return vec3(s * v.x, s * v.y, s * v.z); }
	explicit operator uint() const { return (uint) (s * v.x); }
};
struct lazy4
{
	float s;
	vec4  v;
	operator vec4() const { return vec4(s * v.x, s * v.y, s * v.z, s * v.w); }
};
inline lazy3 operator*(float s, const vec3 &v) { return lazy3{s, v}; }
inline lazy3 operator*(const vec3 &v, float s) { return lazy3{s, v}; }
inline lazy3 operator*(const vec3 &v, int s) { return lazy3{(float) s, v}; }
inline lazy4 operator*(float s, const vec4 &v) { return lazy4{s, v}; }
inline float mul_add(float a, float b, float c) { return g_pinned ? fmaf(a, b, c) : a * b + c; }
inline vec3  operator+(const vec3 &a, const lazy3 &p) { return vec3(mul_add(p.s, p.v.x, a.x), mul_add(p.s, p.v.y, a.y), mul_add(p.s, p.v.z, a.z)); }
inline vec3  operator+(const lazy3 &p, const vec3 &a) { return a + p; }
inline vec4  operator+(const vec4 &a, const lazy4 &p)
{
	return vec4(mul_add(p.s, p.v.x, a.x), mul_add(p.s, p.v.y, a.y), mul_add(p.s, p.v.z, a.z), mul_add(p.s, p.v.w, a.w));
}

// ---- vector arithmetic -----------------------------------------------------------------------------------------------------------------------
inline vec3 operator-(const vec3 &a) { return vec3(-a.x, -a.y, -a.z); }
inline vec3 operator+(const vec3 &a, const vec3 &b) { return vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline vec3 operator-(const vec3 &a, const vec3 &b) { return vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline vec3 operator*(const vec3 &a, const vec3 &b) { return vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline vec3 operator/(const vec3 &a, const vec3 &b) { return vec3(a.x / b.x, a.y / b.y, a.z / b.z); }
inline vec3 operator+(const vec3 &a, float s) { return vec3(a.x + s, a.y + s, a.z + s); }
inline vec3 operator-(const vec3 &a, float s) { return vec3(a.x - s, a.y - s, a.z - s); }
inline vec3 operator/(const vec3 &a, float s) { return vec3(a.x / s, a.y / s, a.z / s); }
inline vec3 operator-(float s, const vec3 &a) { return vec3(s - a.x, s - a.y, s - a.z); }
inline vec3 operator/(float s, const vec3 &a) { return vec3(s / a.x, s / a.y, s / a.z); }
// int vectors with floats: the int operand is converted to float first (GLSL 4.1.10)
inline vec3 operator*(const ivec3 &k, float s) { return vec3((float) k.x * s, (float) k.y * s, (float) k.z * s); }
inline vec3 operator*(const vec3 &a, const ivec3 &k) { return vec3(a.x * (float) k.x, a.y * (float) k.y, a.z * (float) k.z); }
inline vec3 operator-(const ivec3 &k, const vec3 &a) { return vec3((float) k.x - a.x, (float) k.y - a.y, (float) k.z - a.z); }
inline ivec3 operator+(const ivec3 &a, const ivec3 &b) { return ivec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline ivec3 operator-(const ivec3 &a, int s) { return ivec3(a.x - s, a.y - s, a.z - s); }
inline uvec3 operator*(const uvec3 &a, const ivec3 &b) { return uvec3(a.x * (uint) b.x, a.y * (uint) b.y, a.z * (uint) b.z); }

// ---- builtins: GLSL specification semantics ---------------------------------------------------------------------------------------------------
inline float min(float x, float y)
{
	if (g_pinned && x != x)
		return y; // DESIGN.md section 3, "axis-parallel rays": a NaN (0 * inf) never limits the skip
	if (g_pinned && y != y)
		return x;
	return (y < x) ? y : x;
}
inline float max(float x, float y) { return (x < y) ? y : x; }
inline int   min(int x, int y) { return (y < x) ? y : x; }
inline int   max(int x, int y) { return (x < y) ? y : x; }
inline uint  min(uint x, uint y) { return (y < x) ? y : x; }
inline uint  max(uint x, uint y) { return (x < y) ? y : x; }
inline uint  max(int x, uint y) { return max((uint) x, y); } // the int operand is converted to uint (GLSL 4.1.10)
inline float clamp(float x, float lo, float hi) { return min(max(x, lo), hi); }
inline vec3  min(const vec3 &a, const vec3 &b) { return vec3(min(a.x, b.x), min(a.y, b.y), min(a.z, b.z)); }
inline vec3  max(const vec3 &a, const vec3 &b) { return vec3(max(a.x, b.x), max(a.y, b.y), max(a.z, b.z)); }
inline ivec3 min(const ivec3 &a, const ivec3 &b) { return ivec3(min(a.x, b.x), min(a.y, b.y), min(a.z, b.z)); }
inline vec3  clamp(const vec3 &v, float lo, float hi) { return vec3(clamp(v.x, lo, hi), clamp(v.y, lo, hi), clamp(v.z, lo, hi)); }
inline ivec3 clamp(const ivec3 &v, const ivec3 &lo, const ivec3 &hi)
{
	return ivec3(min(max(v.x, lo.x), hi.x), min(max(v.y, lo.y), hi.y), min(max(v.z, lo.z), hi.z));
}
inline float step(float edge, float x) { return (x < edge) ? 0.0f : 1.0f; }
inline vec3  step(float edge, const vec3 &v) { return vec3(step(edge, v.x), step(edge, v.y), step(edge, v.z)); }
inline float sign(float x) { return (x > 0.0f) ? 1.0f : ((x < 0.0f) ? -1.0f : 0.0f); }
inline vec3  sign(const vec3 &v) { return vec3(sign(v.x), sign(v.y), sign(v.z)); }
inline float ceil(float x) { return ceilf(x); }
inline vec3  ceil(const vec3 &v) { return vec3(ceilf(v.x), ceilf(v.y), ceilf(v.z)); }
inline float pow(float x, float y) { return powf(x, y); }
inline float sqrt(float x) { return sqrtf(x); }

inline bool  any(const bvec3 &b) { return b.x || b.y || b.z; }
inline bvec3 lessThanEqual(const vec3 &a, const vec3 &b) { return bvec3(a.x <= b.x, a.y <= b.y, a.z <= b.z); }
inline bvec3 greaterThanEqual(const vec3 &a, const vec3 &b) { return bvec3(a.x >= b.x, a.y >= b.y, a.z >= b.z); }
inline bvec3 greaterThanEqual(const ivec3 &a, const ivec3 &b) { return bvec3(a.x >= b.x, a.y >= b.y, a.z >= b.z); }
inline bvec3 greaterThanEqual(const uvec3 &a, const ivec3 &b) { return bvec3(a.x >= (uint) b.x, a.y >= (uint) b.y, a.z >= (uint) b.z); }
inline bvec3 notEqual(const ivec3 &a, const ivec3 &b) { return bvec3(a.x != b.x, a.y != b.y, a.z != b.z); }

// length(): only the gradient calls it by this name; DESIGN.md section 3 pins sqrt((x*x + y*y) + z*z) there in both modes
inline float length(const vec3 &v) { return sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z); }
// the integrator's norm (normalize, distance): sqrt(fma(z, z, fma(y, y, x * x))) when pinned
inline float norm_integrator(const vec3 &v) { return g_pinned ? sqrtf(fmaf(v.z, v.z, fmaf(v.y, v.y, v.x * v.x))) : length(v); }
inline vec3  normalize(const vec3 &v)
{
	const float n = norm_integrator(v);
	return vec3(v.x / n, v.y / n, v.z / n);
}
inline float distance(const vec3 &a, const vec3 &b) { return norm_integrator(a - b); }

// ---- mat4, column-major -------------------------------------------------------------------------------------------------------------------
struct mat4
{
	float m[16];
};
inline vec4 operator*(const mat4 &M, const vec4 &v)
{
	const float *m = M.m;
	vec4         r;
	float *      o = &r.x;
	for (int i = 0; i < 4; ++i)
		o[i] = g_pinned ? fmaf(m[12 + i], v.w, fmaf(m[8 + i], v.z, fmaf(m[4 + i], v.y, m[i] * v.x))) :
		                  ((m[i] * v.x + m[4 + i] * v.y) + m[8 + i] * v.z) + m[12 + i] * v.w;
	return r;
}
// `A * B * C * v` parses as ((A * B) * C) * v; DESIGN.md section 3 pins gl_FragDepth as A * (B * (C * v)), three matrix-vector products.
// The product of matrices is therefore kept as a list and applied to the vector from the right.
struct matchain
{
	const mat4 *f[4];
	int         n;
};
inline matchain operator*(const mat4 &a, const mat4 &b) { return matchain{{&a, &b, nullptr, nullptr}, 2}; }
inline matchain operator*(matchain c, const mat4 &b)
{
	c.f[c.n++] = &b;
	return c;
}
inline vec4 operator*(const matchain &c, const vec4 &v)
{
	vec4 r = v;
	for (int i = c.n - 1; i >= 0; --i)
		r = *c.f[i] * r;
	return r;
}

// ---- resources over raw bytes -------------------------------------------------------------------------------------------------------------
struct image3D      { uint8_t *p; int w, h, d; };       // R8_UNORM storage image
struct uimage3D     { uint8_t *p; int w, h, d; };       // R8_UINT storage image
struct sampler3D    { const uint8_t *p; int w, h, d; }; // R8_UNORM, LINEAR, CLAMP_TO_EDGE
struct usampler3D   { const uint8_t *p; int w, h, d; }; // R8_UINT, texelFetch only
struct sampler2D    { const uint8_t *p; int w, h; };    // RGBA8_UNORM, NEAREST, CLAMP_TO_EDGE
struct subpassInput { float v; };                       // the scene depth of this fragment

inline uvec3 gl_GlobalInvocationID;

template <class I>
inline bool inside(const I &im, const ivec3 &p) { return p.x >= 0 && p.y >= 0 && p.z >= 0 && p.x < im.w && p.y < im.h && p.z < im.d; }
template <class I>
inline size_t texel_index(const I &im, int x, int y, int z) { return ((size_t) z * (size_t) im.h + (size_t) y) * (size_t) im.w + (size_t) x; }

inline ivec3 imageSize(const image3D &im) { return ivec3(im.w, im.h, im.d); }
inline ivec3 imageSize(const uimage3D &im) { return ivec3(im.w, im.h, im.d); }
inline ivec3 textureSize(const sampler3D &s, int) { return ivec3(s.w, s.h, s.d); }
inline ivec3 textureSize(const usampler3D &s, int) { return ivec3(s.w, s.h, s.d); }

inline float unorm8(uint8_t b) { return (float) b / 255.0f; }
// an access outside the image: the load returns zero and the store is dropped (robust access); the shaders never do it
inline vec4 imageLoad(const image3D &im, const ivec3 &p) { return vec4(inside(im, p) ? unorm8(im.p[texel_index(im, p.x, p.y, p.z)]) : 0.0f, 0.0f, 0.0f, 1.0f); }
inline uvec4 imageLoad(const uimage3D &im, const ivec3 &p) { return uvec4(inside(im, p) ? im.p[texel_index(im, p.x, p.y, p.z)] : 0u, 0u, 0u, 1u); }
inline void imageStore(const image3D &im, const ivec3 &p, const vec4 &v)
{
	if (inside(im, p))
		im.p[texel_index(im, p.x, p.y, p.z)] = (uint8_t) rintf(clamp(v.x, 0.0f, 1.0f) * 255.0f);
}
inline void imageStore(const uimage3D &im, const ivec3 &p, const uvec4 &v)
{
	if (inside(im, p))
		im.p[texel_index(im, p.x, p.y, p.z)] = (uint8_t) min(v.x, 255u);
}
inline void imageStore(const uimage3D &im, const ivec3 &p, const ivec4 &v) { imageStore(im, p, uvec4((uint) max(v.x, 0))); }
inline uvec4 texelFetch(const usampler3D &s, const ivec3 &p, int) { return uvec4(inside(s, p) ? s.p[texel_index(s, p.x, p.y, p.z)] : 0u, 0u, 0u, 1u); }
inline vec4 subpassLoad(const subpassInput &s) { return vec4(s.v, 0.0f, 0.0f, 1.0f); }

inline int iclamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

struct filter_axis
{
	int   i0, i1;
	float w;
};
inline filter_axis linear_axis(float s, int size)
{
	const float u = g_pinned ? fmaf(s, (float) size, -0.5f) : s * (float) size - 0.5f;
	const float f = floorf(u);
	const int   i = (int) f;
	return filter_axis{iclamp(i, 0, size - 1), iclamp(i + 1, 0, size - 1), u - f};
}
inline vec4 texture(const sampler3D &t, const vec3 &pos)
{
	const filter_axis X = linear_axis(pos.x, t.w), Y = linear_axis(pos.y, t.h), Z = linear_axis(pos.z, t.d);
	float             r;
	if (g_pinned)
	{ // the eight BYTES blended as fma(w, b - a, a) along x, y, z; scaled by 1 / 255 once
		const float b000 = t.p[texel_index(t, X.i0, Y.i0, Z.i0)], b100 = t.p[texel_index(t, X.i1, Y.i0, Z.i0)];
		const float b010 = t.p[texel_index(t, X.i0, Y.i1, Z.i0)], b110 = t.p[texel_index(t, X.i1, Y.i1, Z.i0)];
		const float b001 = t.p[texel_index(t, X.i0, Y.i0, Z.i1)], b101 = t.p[texel_index(t, X.i1, Y.i0, Z.i1)];
		const float b011 = t.p[texel_index(t, X.i0, Y.i1, Z.i1)], b111 = t.p[texel_index(t, X.i1, Y.i1, Z.i1)];
		const float c00 = fmaf(X.w, b100 - b000, b000), c10 = fmaf(X.w, b110 - b010, b010);
		const float c01 = fmaf(X.w, b101 - b001, b001), c11 = fmaf(X.w, b111 - b011, b011);
		const float c0 = fmaf(Y.w, c10 - c00, c00), c1 = fmaf(Y.w, c11 - c01, c01);
		r = fmaf(Z.w, c1 - c0, c0) * (1.0f / 255.0f);
	}
	else
	{ // Vulkan specification, "Texel Filtering": the weighted sum over the eight texels, z outermost, x innermost
		const int   zi[2] = {Z.i0, Z.i1}, yi[2] = {Y.i0, Y.i1}, xi[2] = {X.i0, X.i1};
		const float wz[2] = {1.0f - Z.w, Z.w}, wy[2] = {1.0f - Y.w, Y.w}, wx[2] = {1.0f - X.w, X.w};
		r = 0.0f;
		for (int k = 0; k < 2; ++k)
			for (int j = 0; j < 2; ++j)
				for (int i = 0; i < 2; ++i)
					r = r + ((wx[i] * wy[j]) * wz[k]) * unorm8(t.p[texel_index(t, xi[i], yi[j], zi[k])]);
	}
	return vec4(r, 0.0f, 0.0f, 1.0f);
}
inline vec4 texture(const sampler2D &t, const vec2 &st)
{
	const int      i = iclamp((int) floorf(st.x * (float) t.w), 0, t.w - 1), j = iclamp((int) floorf(st.y * (float) t.h), 0, t.h - 1);
	const uint8_t *c = t.p + ((size_t) j * (size_t) t.w + (size_t) i) * 4;
	return vec4(unorm8(c[0]), unorm8(c[1]), unorm8(c[2]), unorm8(c[3]));
}
} // namespace glsl

// storage qualifier of a function parameter (`const in vec3 v`): nothing in C++; `discard`: flag, then leave main()
#define in
#define discard                        \
	do                                 \
	{                                  \
		vkv_fragment_discarded = true; \
		return;                        \
	} while (0)
