// median27_network.hpp — the compare-exchange selection network of the 3x3x3 median (filter.hip), written once as templates
// over the element type T and its two operations: lo(a, b) = the smaller, hi(a, b) = the larger.  filter.hip instantiates it on two 16-bit
// fields per dword (v_pk_min_u16 / v_pk_max_u16: two voxels per instruction); tests/median27_driver.cpp instantiates it on 64-bit bit
// slices (AND / OR) and runs all 2^27 zero/one inputs, which by the zero-one principle proves it for every input.
//
// The 27 values are taken as three planes of nine (the kernel: the y-z plane of each of the three x columns), every plane as three triples
// (the three y neighbours of one z slice).  The stages are the pieces the kernel reuses: a sorted triple serves the three z outputs that
// see its slice, a sorted plane serves the three x outputs that see its column.
//   sort3            3 compare-exchanges                                   (per triple)
//   merge_triples    16 compare-exchanges: three sorted triples -> sorted 9 (per plane; with sort3 the 25 of the optimal 9-sorter)
//   median_of_sorted 69 min / max: rank 13 of three sorted nines          (per output)
// No stage has a data-dependent branch or index, so everything stays in registers.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VKV_NET_FN __host__ __device__ __forceinline__
#else
#define VKV_NET_FN inline
#endif

namespace vkv
{
template <class T, class Ops>
VKV_NET_FN void net_cx(T &a, T &b, const Ops &op)        // compare-exchange: a <= b afterwards
{
	const T l = op.lo(a, b), h = op.hi(a, b);
	a = l, b = h;
}

template <class T, class Ops>
VKV_NET_FN void sort3(T &a, T &b, T &c, const Ops &op)
{
	net_cx(a, b, op), net_cx(b, c, op), net_cx(a, b, op);
}

// v[0..2], v[3..5], v[6..8] each ascending -> v[0..8] ascending
template <class T, class Ops>
VKV_NET_FN void merge_triples(T (&v)[9], const Ops &op)
{
	// the columns of the 3 x 3 matrix of sorted rows
	net_cx(v[0], v[3], op), net_cx(v[3], v[6], op), net_cx(v[0], v[3], op);
	net_cx(v[1], v[4], op), net_cx(v[4], v[7], op), net_cx(v[1], v[4], op);
	net_cx(v[2], v[5], op), net_cx(v[5], v[8], op), net_cx(v[2], v[5], op);
	// the anti-diagonals
	net_cx(v[1], v[3], op), net_cx(v[5], v[7], op), net_cx(v[2], v[6], op), net_cx(v[4], v[6], op);
	net_cx(v[2], v[4], op), net_cx(v[2], v[3], op), net_cx(v[5], v[6], op);
}

// The element of rank 13 (0-based) of the 27 values of three ascending nines.  Index by index the three lists are ordered into l <= m <= h
// (again three ascending lists); with the zero counts p >= q >= r of l, m, h in a zero/one input the median is zero iff p + q + r >= 14,
// and the minimal such (p, q, r) with 9 >= p >= q >= r are the fifteen terms below: median = min over them of
// max(l[p - 1], m[q - 1], h[r - 1]) (a count of 0 drops its operand).  Only l[4..8], m[2..6] and h[0..3] occur.
template <class T, class Ops>
VKV_NET_FN T median_of_sorted(const T (&a)[9], const T (&b)[9], const T (&c)[9], const Ops &op)
{
	auto min3 = [&](int i) { return op.lo(op.lo(a[i], b[i]), c[i]); };
	auto max3 = [&](int i) { return op.hi(op.hi(a[i], b[i]), c[i]); };
	auto med3 = [&](int i) { return op.hi(op.lo(a[i], b[i]), op.lo(op.hi(a[i], b[i]), c[i])); };
	const T l4 = min3(4), l5 = min3(5), l6 = min3(6), l7 = min3(7), l8 = min3(8);
	const T m2 = med3(2), m3 = med3(3), m4 = med3(4), m5 = med3(5), m6 = med3(6);
	const T h0 = max3(0), h1 = max3(1), h2 = max3(2), h3 = max3(3);
	// (p; q, r): (9; 5,0 4,1 3,2)  (8; 6,0 5,1 4,2 3,3)  (7; 7,0 6,1 5,2 4,3)  (6; 6,2 5,3 4,4)  (5; 5,4)
	const T t9 = op.hi(l8, op.lo(op.lo(m4, op.hi(m3, h0)), op.hi(m2, h1)));
	const T t8 = op.hi(l7, op.lo(op.lo(m5, op.hi(m4, h0)), op.lo(op.hi(m3, h1), op.hi(m2, h2))));
	const T t7 = op.hi(l6, op.lo(op.lo(m6, op.hi(m5, h0)), op.lo(op.hi(m4, h1), op.hi(m3, h2))));
	const T t6 = op.hi(l5, op.lo(op.lo(op.hi(m5, h1), op.hi(m4, h2)), op.hi(m3, h3)));
	const T t5 = op.hi(l4, op.hi(m4, h3));
	return op.lo(op.lo(op.lo(t9, t8), op.lo(t7, t6)), t5);
}

// the whole network: v[9 * plane + 3 * triple + i]
template <class T, class Ops>
VKV_NET_FN T median27(const T (&v)[27], const Ops &op)
{
	T s[3][9];
	for (int p = 0; p < 3; ++p)
	{
		for (int i = 0; i < 9; ++i)
			s[p][i] = v[9 * p + i];
		for (int t = 0; t < 3; ++t)
			sort3(s[p][3 * t], s[p][3 * t + 1], s[p][3 * t + 2], op);
		merge_triples(s[p], op);
	}
	return median_of_sorted(s[0], s[1], s[2], op);
}
}        // namespace vkv
