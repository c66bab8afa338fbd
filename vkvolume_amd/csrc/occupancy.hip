// occupancy.hip — the occupancy map (vkv_occupancy_map, shaders/occupancy_map.comp:45-73: a cell is OCCUPIED = 0 when one of its voxels has
// alpha > 0, else EMPTY = 255) and the occupied-voxel count of the analytic transfer function (vkv_occupied_voxel_count).  Replaces
// ComputeDistanceMap::computeOccupancy (src/compute_distance_map.cpp) and ComputeOccupiedVoxelCount.  Byte streaming; no MFMA.
//
// k_occupancy_map_waves<GRAD, ROWS, CRB> builds the whole map for every width >= 4 with the gradient off or precomputed.
// k_occupancy_map<GRAD>, a workgroup per run of cells of a cell row, takes the rest: widths below 4, the on-the-fly gradient (GRAD = 2,
// use_gradient without a gradient map), and the cell range of a region update (launch_occupancy_map_cells), where every cell of the range is
// written and no other.
#include <algorithm>

#include "launchers.hpp"

using namespace vkv;

// alpha > 0 is a pure function of (gradient texel, intensity texel) of the NEAREST-sampled TF texture, so the
// 256x256 alpha channel is first reduced to a 1-bit table (8 KiB) that every block stages in LDS.
__global__ void __launch_bounds__(256) k_tf_bits(const uint8_t *__restrict__ tf_rgba8, uint32_t *__restrict__ bits)
{
	const uint32_t w = blockIdx.x * 256 + threadIdx.x;        // 2048 words
	if (w >= 2048)
		return;
	uint32_t v = 0;
	for (int i = 0; i < 32; ++i)
		v |= (tf_rgba8[((size_t) w * 32 + i) * 4 + 3] > 0 ? 1u : 0u) << i;
	bits[w] = v;
}

// Which INTENSITY bytes can be occupied at all (alpha > 0 for some gradient byte): 256 bits behind the bit table (words 2048..2055).  A voxel
// whose intensity is not among them is empty whatever its gradient: k_occupancy_map_waves tests the lowest such byte against whole batches of
// volume dwords before it touches the gradient map or the table.
__global__ void __launch_bounds__(256) k_tf_columns(uint32_t *__restrict__ bits)
{
	const uint32_t v = threadIdx.x;        // intensity byte = texture column
	uint32_t       any = 0;
	for (uint32_t g = 0; g < 256; ++g)
		any |= bits[g * 8u + (v >> 5)];
	const unsigned long long m = __builtin_amdgcn_ballot_w64(((any >> (v & 31u)) & 1u) != 0u);
	if ((v & 63u) == 0u)
		bits[2048u + (v >> 5)] = (uint32_t) m, bits[2048u + (v >> 5) + 1u] = (uint32_t) (m >> 32);
}

// Block = 256 threads = 256 consecutive voxels in x of one cell row (cy, cz); it walks the by*bz voxel rows of
// that cell row, every load being a coalesced 64-byte segment per wave, ORs "occupied" into one LDS flag per cell.
// GRAD: 0 = use_gradient false (gradient = 1.0), 1 = precomputed map, 2 = on-the-fly tetrahedron.
template <int GRAD>
__global__ void __launch_bounds__(256) k_occupancy_map(const uint8_t *__restrict__ vol, const uint8_t *__restrict__ grad,
                                                       const uint32_t *__restrict__ tf_bits, uint8_t *__restrict__ map, int W, int H, int D,
                                                       int mw, int mh, int md, int bx, int by, int bz, float modifier, uint32_t blocks_x,
                                                       int cx0, int cy0, int cz0, int cx1)
{
	__shared__ uint32_t s_bits[2048];
	__shared__ uint32_t s_cell[256];
	for (int i = threadIdx.x; i < 2048; i += 256)
		s_bits[i] = tf_bits[i];
	s_cell[threadIdx.x] = 0;
	__syncthreads();

	// the grid covers the cells [cx0, cx1) of the cell rows cy0 .. and slices cz0 .. (the whole map, or the cells of a region update: every
	// cell is written, OCCUPIED or EMPTY)
	const uint32_t bxi = blockIdx.x % blocks_x;
	const int      cy = cy0 + (int) (blockIdx.x / blocks_x), cz = cz0 + (int) blockIdx.y;        // grid = (x blocks * cell rows, cell slices)
	// the block covers cells [c0, c0 + cells_per_block) of this cell row
	const int cells_per_block = 256 / bx > 0 ? 256 / bx : 1;
	const int c0              = cx0 + (int) bxi * cells_per_block;
	const int x0              = c0 * bx;
	const int span            = cells_per_block * bx;        // voxels handled per pass (<= 256 unless bx > 256)
	const int y_end = min((cy + 1) * by, H), z_end = min((cz + 1) * bz, D);

	uint32_t occ = 0;
	for (int lx = threadIdx.x; lx < span; lx += 256)
	{
		const int x = x0 + lx;
		if (x >= W)
			break;
		occ = 0;
		for (int z = cz * bz; z < z_end; ++z)
			for (int y = cy * by; y < y_end; ++y)
			{
				const size_t   o = vidx(x, y, z, W, H);
				const uint32_t v = vol[o];
				uint32_t       g;
				if (GRAD == 1)
					g = grad[o];        // unorm8 byte: NEAREST lookup of b/255 lands on texel b
				else if (GRAD == 2)
					g = (uint32_t) tf_texel(gradient_on_the_fly(vol, W, H, D, x, y, z, modifier));
				else
					g = 255;        // gradient = 1.0 -> texel 255
				const uint32_t bit = g * 256 + v;
				occ |= (s_bits[bit >> 5] >> (bit & 31)) & 1u;
			}
		if (occ)
			s_cell[lx / bx] = 1;        // benign race: every writer stores 1
	}
	__syncthreads();
	const int c = c0 + (int) threadIdx.x;
	if ((int) threadIdx.x < cells_per_block && c < cx1)
		map[vidx(c, cy, cz, mw, mh)] = s_cell[threadIdx.x] ? 0 : 255;        // OCCUPIED = 0, EMPTY = 255
}

// Any block width at streaming rate (round 5; the sweep's block sizes 2, 3, 5, 6 - and 3 is where the reference publishes its best frame
// rates).  What the kernel above loses on small or odd blocks: a workgroup per cell row streams by * bz voxel rows (9 for a 3^3
// block: 18 KB) for 8 KB of staged bit table, meets at barriers for every cell row, and fetches rows in eights, so a 9-row cell pays for 16.
//   * The map is first filled with EMPTY (255) and the kernel only ever stores OCCUPIED (0): any number of lanes may then hit the same cell
//     in any order, so nothing has to be aligned to cells and nothing is exchanged.
//   * Every WAVE is on its own: it owns 64 consecutive dwords (256 voxels) in x and walks `cy_per_wave` consecutive cell rows of them; the
//     bit table is staged once per workgroup, i.e. once per >= 256 KB of voxels, and that is the kernel's only barrier.
//   * A wave fetches exactly ROWS voxel rows per batch - ROWS / CRB rows of each of CRB cell rows (the launcher picks ROWS from {8, 9, 10, 12}
//     so that by * bz rows leave the fewest idle slots: 9 -> 9, 16 -> 8, 25 -> 27, 36 -> 36, 49 -> 50; cells of fewer than eight rows are
//     taken CRB = 2, 4 or 8 cell rows at a time: a 2^3 block's four rows two cell rows at a time).
//   * Short circuit: the VOLUME dwords of a batch come first.  If no byte of them reaches the lowest intensity the transfer function gives any
//     alpha to (k_tf_columns; four bytes per SWAR test), every voxel of the batch is empty whatever its gradient: the wave goes on to the next
//     batch without reading the gradient map or the table - on the bench volume that is most batches, i.e. close to half the bytes
//     occupancy_map.comp reads.  Otherwise the gradient rows follow and every voxel is looked up (same result either way: the test is exact).
//   * A lane ORs the occupied bits of its four voxels over a cell row's rows and stores a 0 into the cells of the voxels that have one (a
//     lane's four voxels lie in the same cells in every cell row: the x -> cell division is done once).
// a wave-uniform 64-bit value moved into scalar registers (the compiler does not always see the uniformity through the loops' counters)
__device__ __forceinline__ size_t uniform_u64(size_t x)
{
	const uint32_t lo = (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) x), hi = (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) (x >> 32));
	return ((size_t) hi << 32) | lo;
}

template <int GRAD, int ROWS, int CRB>
__global__ void __launch_bounds__(256) k_occupancy_map_waves(const uint8_t *__restrict__ vol, const uint8_t *__restrict__ grad, const uint32_t *__restrict__ tf_bits,
                                                             uint8_t *__restrict__ map, int W, int H, int D, int mw, int mh, int bx, int by, int bz, uint32_t spans_x,
                                                             int cy_per_wave)
{
	__shared__ uint32_t s_bits[2048];
	for (int i = threadIdx.x; i < 2048; i += 256)
		s_bits[i] = tf_bits[i];
	// lowest intensity byte with any alpha (256: none - the map stays empty; 0: no short circuit possible)
	uint32_t vmin = 256u;
	for (int w = 7; w >= 0; --w)
	{
		const uint32_t m = tf_bits[2048 + w];        // wave-uniform scalar loads
		if (m)
			vmin = (uint32_t) w * 32u + (uint32_t) __builtin_ctz(m);
	}
	__syncthreads();
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const uint32_t task = blockIdx.x * 4u + wave;        // (span of 64 dwords in x, group of cell rows); blockIdx.y = cell slice
	const int      xd = (int) (task % spans_x) * 64 + (int) lane, cy0 = (int) (task / spans_x) * cy_per_wave, cz = (int) blockIdx.y;
	if (cy0 >= mh || xd * 4 >= W || vmin == 256u)
		return;
	// the lane's byte offset inside a row: scalar row base + 32-bit lane offset per load.  The last lane of an odd width (x + 4 > W) loads the
	// row's last four bytes instead and shifts them down (row_dword); its voxels past the row are masked out of the result
	const uint32_t xo_ = (uint32_t) xd * 4u, xo = min(xo_, (uint32_t) (W - 4)), shr = (xo_ - xo) * 8u;
	const uint32_t valid   = xo_ + 4u <= (uint32_t) W ? 0xfu : (1u << ((uint32_t) W - xo_)) - 1u;
	const bool     shifted = __builtin_amdgcn_ballot_w64(shr != 0u) != 0ull;        // wave-uniform: only the wave that holds the row's end
	// "some byte of x is >= vmin" for four bytes at once: byte + (256 - vmin) carries out of its eight bits.  The low seven bits are added
	// per byte (no carry between bytes: 127 + 127 < 256), the carry out of bit 7 is then majority(byte's bit 7, the constant's bit 7, the
	// sum's bit 7), i.e. an OR or an AND with the constant's bit 7 known
	const uint32_t cadd = 256u - vmin, c_hi = cadd >> 7, c_lo4 = (cadd & 127u) * 0x01010101u;
	// the cells of this lane's four voxels: cell0 = the first voxel's, step bit i = voxel i lies in the next cell (one store per cell)
	uint32_t cell0 = (uint32_t) (4 * xd) / (uint32_t) bx, step = 0u;
	{
		uint32_t in = (uint32_t) (4 * xd) - cell0 * (uint32_t) bx;
#pragma unroll
		for (int i = 1; i < 4; ++i)
			if (++in == (uint32_t) bx)
				in = 0, step |= 1u << i;
	}
	const int    z_end = min((cz + 1) * bz, D), nz = z_end - cz * bz;
	// a map may have more cell rows / slices than the volume fills (map extent > ceil(extent / block), e.g. 16^3 voxels under a 7^3 map:
	// block 3, cells 6 of y and z lie outside): those cells hold no voxel and stay EMPTY, like in the workgroup-per-cell-row kernel
	const int    cy_end = min(min(cy0 + cy_per_wave, mh), (H + by - 1) / by);
	if (nz <= 0 || cy0 >= cy_end)
		return;
	const size_t zs = (size_t) H * (size_t) W;
	for (int cy = cy0; cy < cy_end; cy += CRB)
	{
		uint32_t occ[CRB];
#pragma unroll
		for (int k = 0; k < CRB; ++k)
			occ[k] = 0;
		const int ny     = min((cy + 1) * by, H) - cy * by;        // CRB == 1: rows of this cell row in y (whole cells otherwise)
		const int n_rows = CRB == 1 ? ny * nz : ROWS;
		int       ry = 0, rz = 0;        // CRB == 1: the (y, z) of the next row inside the cell row (wave-uniform counters instead of a division per load)
		for (int r0 = 0; r0 < n_rows; r0 += ROWS)
		{
			size_t   row[ROWS];
			uint32_t v4[ROWS];
#pragma unroll
			for (int j = 0; j < ROWS; ++j)
			{
				if (CRB == 1)
				{
					row[j] = (size_t) (cz * bz + rz) * zs + (size_t) (cy * by + ry) * (size_t) W;
					if (!(rz == nz - 1 && ry == ny - 1))        // the tail repeats the last row (idempotent OR; the line is in L1)
					{
						if (++ry == ny)
							ry = 0, ++rz;
					}
				}
				else
				{        // by * bz = ROWS / CRB rows per cell row; the rows a ragged last cell row / slice does not have repeat its last one
					constexpr int kPer = ROWS / CRB;
					const int     c = min(cy + j / kPer, cy_end - 1), r = j % kPer;        // (a group's last batch repeats its last cell row)
					row[j]          = (size_t) (cz * bz + min(r / by, nz - 1)) * zs + (size_t) min(c * by + r % by, H - 1) * (size_t) W;
				}
				row[j] = uniform_u64(row[j]);        // wave-uniform by construction: a scalar base for the two loads of this row
				v4[j]  = load_u32_any(vol + row[j] + xo);
				if (shifted)
					v4[j] >>= shr;
			}
			if (vmin != 0u)
			{
				uint32_t acc = 0;
#pragma unroll
				for (int j = 0; j < ROWS; ++j)
				{
					const uint32_t sum = (v4[j] & 0x7f7f7f7fu) + c_lo4;
					acc |= c_hi ? (v4[j] | sum) : (v4[j] & sum);
				}
				if (__builtin_amdgcn_ballot_w64((acc & 0x80808080u) != 0u) == 0ull)
					continue;        // the whole batch of the whole wave is below the transfer function's threshold
			}
			uint32_t g4[ROWS];
#pragma unroll
			for (int j = 0; j < ROWS; ++j)
			{
				g4[j] = GRAD == 1 ? load_u32_any(grad + row[j] + xo) : 0xffffffffu;
				if (GRAD == 1 && shifted)
					g4[j] >>= shr;
			}
#pragma unroll
			for (int j = 0; j < ROWS; ++j)
#pragma unroll
				for (int i = 0; i < 4; ++i)
				{
					const uint32_t bit = ((g4[j] >> (8 * i)) & 255u) * 256u + ((v4[j] >> (8 * i)) & 255u);
					occ[CRB == 1 ? 0 : j / (ROWS / CRB)] |= ((s_bits[bit >> 5] >> (bit & 31u)) & 1u) << i;
				}
		}
#pragma unroll
		for (int k = 0; k < CRB; ++k)
		{
			occ[k] &= valid;        // (the voxels a row's last lane holds past the row's end)
			if (cy + k >= cy_end || occ[k] == 0u)
				continue;
			uint8_t *out = map + ((size_t) cz * mh + (size_t) (cy + k)) * (size_t) mw;
			// OR the bits of the voxels that share a cell, then one store per occupied cell
			uint32_t c = cell0, any = 0u;
#pragma unroll
			for (int i = 0; i < 4; ++i)
			{
				if (i > 0 && ((step >> i) & 1u))
				{
					if (any)
						out[c] = 0;        // OCCUPIED
					++c, any = 0u;
				}
				any |= (occ[k] >> i) & 1u;
			}
			if (any)
				out[c] = 0;
		}
	}
}

// ---------------------------------------------------------------------------------------------
// Occupied-voxel count (shaders/occupied_voxel_count.comp + occupied_voxel_count_reduce.comp)
// ---------------------------------------------------------------------------------------------
// The statistic's alpha is again a pure function of the (gradient byte, intensity byte) pair when the gradient comes
// from the R8_UNORM map: reduce the analytic TF to the same 8 KiB bit table the occupancy pass uses.
__global__ void __launch_bounds__(256) k_tf_bits_analytic(uint32_t *__restrict__ bits, float imin, float iinv, float gmin, float ginv)
{
	const uint32_t w = blockIdx.x * 256 + threadIdx.x;        // 2048 words, 32 intensity texels each
	if (w >= 2048)
		return;
	const uint32_t g = w >> 3;
	uint32_t       v = 0;
	for (uint32_t i = 0; i < 32; ++i)
		v |= (analytic_occupied(unorm8((w & 7u) * 32 + i), unorm8(g), imin, iinv, gmin, ginv) ? 1u : 0u) << i;
	bits[w] = v;
}

// GRAD as in k_occupancy_map.  Each thread walks voxels with a grid stride of whole x rows; a wave counts with
// ballot + popcount, a workgroup adds once to the 64-bit total.
template <int GRAD, int DWORDS>        // DWORDS: 0 = a voxel per lane, 1 = four per lane from aligned dwords (W % 4 == 0), 2 = four per lane at any alignment / width
__global__ void __launch_bounds__(256) k_occupied_voxel_count(const uint8_t *__restrict__ vol, const uint8_t *__restrict__ grad,
                                                              const uint32_t *__restrict__ tf_bits, unsigned long long *__restrict__ total, int W, int H,
                                                              int D, float modifier, float imin, float iinv, float gmin, float ginv, uint32_t blocks_x,
                                                              uint32_t n_row_groups)
{
	__shared__ uint32_t s_bits[2048];
	__shared__ uint32_t s_wave[4];
	for (int i = threadIdx.x; i < 2048; i += 256)
		s_bits[i] = tf_bits[i];
	__syncthreads();
	const uint32_t bx   = blockIdx.x % blocks_x;
	const uint32_t rows = (uint32_t) H * (uint32_t) D;
	uint32_t       n    = 0;
	if (GRAD != 2 && DWORDS)
	{        // dword-aligned rows: one lane tests 4 voxels per load (256 contiguous bytes per wave-load)
		const int      xd     = (int) (bx * 64 + (threadIdx.x & 63));        // dword column
		const uint32_t stride = gridDim.x / blocks_x;
		constexpr int  kBatch = 8;        // row groups fetched together: 16 loads in flight per lane
		// (any width >= 4: the row's last lane reads the row's last four bytes and shifts, row_dword; its voxels past the row do not count)
		const int n_valid = min(4, W - 4 * xd);
		if (xd * 4 < W)
			for (uint32_t rg0 = blockIdx.x / blocks_x; rg0 < n_row_groups; rg0 += stride * kBatch)
			{
				uint32_t v4[kBatch], g4[kBatch];
#pragma unroll
				for (int j = 0; j < kBatch; ++j)
				{
					const uint32_t row = (rg0 + (uint32_t) j * stride) * 4 + (threadIdx.x >> 6);
					const bool     ok  = rg0 + (uint32_t) j * stride < n_row_groups && row < rows;
					const size_t   o   = (size_t) (ok ? row : 0u) * (size_t) W;
					if (DWORDS == 1)
					{
						v4[j] = ok ? reinterpret_cast<const uint32_t *>(vol + o)[xd] : 0u;
						g4[j] = (ok && GRAD == 1) ? reinterpret_cast<const uint32_t *>(grad + o)[xd] : (ok ? 0xffffffffu : 0u);
					}
					else
					{
						v4[j] = ok ? row_dword(vol + o, xd, W) : 0u;
						g4[j] = (ok && GRAD == 1) ? row_dword(grad + o, xd, W) : (ok ? 0xffffffffu : 0u);
					}
				}
#pragma unroll
				for (int j = 0; j < kBatch; ++j)
				{
					const bool ok = rg0 + (uint32_t) j * stride < n_row_groups && (rg0 + (uint32_t) j * stride) * 4 + (threadIdx.x >> 6) < rows;
#pragma unroll
					for (int i = 0; i < 4; ++i)
					{
						const uint32_t bit = ((g4[j] >> (8 * i)) & 255u) * 256u + ((v4[j] >> (8 * i)) & 255u);
						n += (ok && (DWORDS == 1 || i < n_valid)) ? (s_bits[bit >> 5] >> (bit & 31u)) & 1u : 0u;        // per-lane partial sums, reduced below
					}
				}
			}
		for (int o2 = 32; o2 > 0; o2 >>= 1)
			n += (uint32_t) __shfl_xor((int) n, o2);
	}
	else
	{
	const int x = (int) (bx * 64 + (threadIdx.x & 63));
	for (uint32_t rg = blockIdx.x / blocks_x; rg < n_row_groups; rg += gridDim.x / blocks_x)
	{
		const uint32_t row = rg * 4 + (threadIdx.x >> 6);
		bool           occ = false;
		if (x < W && row < rows)
		{
			const int      y = (int) (row % (uint32_t) H), z = (int) (row / (uint32_t) H);
			const size_t   o = vidx(x, y, z, W, H);
			const uint32_t v = vol[o];
			if (GRAD == 2)
				occ = analytic_occupied(unorm8(v), gradient_on_the_fly(vol, W, H, D, x, y, z, modifier), imin, iinv, gmin, ginv);
			else
			{
				const uint32_t bit = (GRAD == 1 ? (uint32_t) grad[o] : 255u) * 256 + v;
				occ                = (s_bits[bit >> 5] >> (bit & 31)) & 1u;
			}
		}
		n += (uint32_t) __popcll(__ballot(occ));        // wave-uniform
	}
	}
	if ((threadIdx.x & 63) == 0)
		s_wave[threadIdx.x >> 6] = n;
	__syncthreads();
	if (threadIdx.x == 0)
		atomicAdd(total, (unsigned long long) s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]);
}

namespace vkv
{

// 255 (EMPTY) into n bytes: 16-byte stores over the aligned body, single bytes at both ends.  The map fill of vkv_update_transfer_function:
// replays of a hipGraph that held the fill as a memset node gave maps that differed from replay to replay, while kernel nodes stay ordered
__global__ void __launch_bounds__(256) k_fill_empty(uint8_t *__restrict__ p, size_t n)
{
	const size_t head = min(n, (size_t) ((16u - ((uintptr_t) p & 15u)) & 15u));
	const size_t body = (n - head) / 16, tail = head + body * 16;
	const size_t tid = (size_t) blockIdx.x * 256 + threadIdx.x, stride = (size_t) gridDim.x * 256;
	if (tid < head)
		p[tid] = 255;
	uint4 *q = reinterpret_cast<uint4 *>(p + head);
	for (size_t i = tid; i < body; i += stride)
		q[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
	if (tid < n - tail)
		p[tail + tid] = 255;
}

// A distance map (or an octant map) back into the occupancy it was made from: every transform keeps the zero set (a cell is its own
// candidate at distance 0, any other is at least 1 away), so byte v -> v == 0 ? OCCUPIED (0) : EMPTY (255).  Same layout as k_fill_empty.
__global__ void __launch_bounds__(256) k_occupancy_of_distance(uint8_t *__restrict__ p, size_t n)
{
	const size_t head = min(n, (size_t) ((16u - ((uintptr_t) p & 15u)) & 15u));
	const size_t body = (n - head) / 16, tail = head + body * 16;
	const size_t tid = (size_t) blockIdx.x * 256 + threadIdx.x, stride = (size_t) gridDim.x * 256;
	if (tid < head)
		p[tid] = p[tid] ? 255 : 0;
	// bit 7 of ((b & 0x7f) + 0x7f) | b is set exactly for the non-zero bytes b (no carries between bytes)
	auto nonzero = [](uint32_t w) { return ((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u) >> 7; };
	uint4 *q = reinterpret_cast<uint4 *>(p + head);
	for (size_t i = tid; i < body; i += stride)
	{
		const uint4 v = q[i];
		q[i]          = make_uint4(nonzero(v.x) * 255u, nonzero(v.y) * 255u, nonzero(v.z) * 255u, nonzero(v.w) * 255u);
	}
	if (tid < n - tail)
		p[tail + tid] = p[tail + tid] ? 255 : 0;
}

static int fill_empty(vkv_ctx *ctx, uint8_t *d_map, size_t n, hipStream_t s, bool by_kernel)
{
	if (by_kernel)
	{
		const size_t blocks = std::min<size_t>(std::max<size_t>(1, (n / 16 + 255) / 256), 4096);
		hipLaunchKernelGGL(k_fill_empty, dim3((uint32_t) blocks), dim3(256), 0, s, d_map, n);
		return check_launch(ctx, "occupancy_map: fill");
	}
	const hipError_t em = hipMemsetAsync(d_map, 255, n, s);
	return em == hipSuccess ? VKV_OK : set_error(ctx, (int) em, "occupancy_map: fill: %s", hipGetErrorString(em));
}

// what the occupancy pass (whole map or a region update's) can take in one launch: the grid of k_occupancy_map
bool occupancy_launch_ok(VkvExtent3D e, VkvExtent3D me)
{
	const int bx = (int) block_of(e.width, me.width), cells_per_block = 256 / bx > 0 ? 256 / bx : 1;
	return (uint64_t) ((me.width + cells_per_block - 1) / cells_per_block) * me.height <= 0xffffffull && me.depth <= 65535u;
}

// d_bits: the bit table in the stream's scratch block (per stream: map updates on different streams do not share it; the caller holds the
// block's lock).  bits_ready: k_tf_build has already left the bit table and its column mask there (vkv_update_transfer_function); d_tf is
// then not read, and the map is filled by a kernel (k_fill_empty)
int launch_occupancy_map(vkv_ctx *ctx, const uint8_t *d_vol, const uint8_t *d_grad, const uint8_t *d_tf, const VkvTransferFunctionUniform *tf,
                         VkvExtent3D e, uint8_t *d_map, VkvExtent3D me, hipStream_t s, uint32_t *d_bits, bool bits_ready)
{
	if (!occupancy_launch_ok(e, me))
		return set_error(ctx, VKV_E_UNSUPPORTED, "occupancy_map: map too large for one launch");
	if (!bits_ready)
	{
		hipLaunchKernelGGL(k_tf_bits, dim3(8), dim3(256), 0, s, d_tf, d_bits);
		hipLaunchKernelGGL(k_tf_columns, dim3(1), dim3(256), 0, s, d_bits);        // words 2048..2055 of the scratch's table area
	}
	// src/compute_distance_map.cpp:110-113
	const int bx = (int) block_of(e.width, me.width), by = (int) block_of(e.height, me.height), bz = (int) block_of(e.depth, me.depth);
	const int      cells_per_block = 256 / bx > 0 ? 256 / bx : 1;
	const uint32_t blocks_x        = (me.width + cells_per_block - 1) / cells_per_block;
	const dim3 grid(blocks_x * me.height, me.depth);
	const int W = (int) e.width, H = (int) e.height, D = (int) e.depth, mw = (int) me.width, mh = (int) me.height, md = (int) me.depth;
	const bool precomputed = tf->use_gradient && d_grad;
	// a map extent above ceil(extent / block) leaves cells without a voxel: EMPTY.  The wave kernel fills the whole map first anyway;
	// k_occupancy_map only visits cells the volume reaches in x, so such a map is filled for it too
	if ((uint64_t) (mw - 1) * bx >= (uint64_t) W || (uint64_t) (mh - 1) * by >= (uint64_t) H || (uint64_t) (md - 1) * bz >= (uint64_t) D)
	{
		const int rc = fill_empty(ctx, d_map, (size_t) me.width * me.height * me.depth, s, bits_ready);
		if (rc != VKV_OK)
			return rc;
	}
	// round 6: any width >= 4 and any alignment (the kernel's loads need none; the last lane of an odd row reads the row's last four bytes)
	const bool dword_ok = e.width >= 4 && (!tf->use_gradient || precomputed);
	if (dword_ok)
	{        // any block width: a wave per 64 dwords (k_occupancy_map_waves)
		const uint32_t spans_x = (uint32_t) (((e.width + 3) / 4 + 63) / 64);
		const int      n_rows  = by * bz;
		int            rows = 8, crb = 1;
		if (n_rows == 1 || n_rows == 2 || n_rows == 4)
			crb = 8 / n_rows;        // eight rows per batch out of 8, 4 or 2 cell rows
		else
		{
			int waste = 1 << 30;
			for (int cand : {8, 9, 10, 12})
			{
				const int w = (n_rows + cand - 1) / cand * cand - n_rows;
				if (w < waste)
					waste = w, rows = cand;
			}
		}
		// cell rows per wave: >= 64 KB of voxels behind a wave's share of the bit table's staging, but at least 32 waves per CU in the launch
		const size_t row_bytes = (size_t) 256 * n_rows * (precomputed ? 2 : 1);
		int          cyw       = (int) std::min<size_t>(std::max<size_t>(1, (64 * 1024 + row_bytes - 1) / row_bytes), me.height);
		const uint64_t want = (uint64_t) 32 * (uint64_t) std::max(1, ctx->cu_count);
		while (cyw > crb && (uint64_t) spans_x * ((me.height + cyw - 1) / cyw) * me.depth < want)
			cyw >>= 1;
		cyw = (cyw + crb - 1) / crb * crb;
		const uint64_t tasks = (uint64_t) spans_x * ((me.height + cyw - 1) / cyw);
		// Always true for blocks of up to 256 voxels in x: occupancy_launch_ok has bounded ceil(mw / cpb) * mh by 2^24 (cpb = 256 / bx cells,
		// so bx * cpb <= 256) and md by 65535, and spans_x = ceil(W / 256) <= ceil(mw * bx / 256) <= ceil(mw / cpb) because W <= mw * bx;
		// tasks <= spans_x * mh follows.  Wider blocks may miss it: they go on to k_occupancy_map, which takes every map that limit admits
		if ((tasks + 3) / 4 <= 0x7fffffffull && me.depth <= 65535u)
		{
			const int rc = fill_empty(ctx, d_map, (size_t) me.width * me.height * me.depth, s, bits_ready);        // EMPTY everywhere; the kernel stores the OCCUPIED cells
			if (rc != VKV_OK)
				return rc;
			const dim3 wgrid((uint32_t) ((tasks + 3) / 4), me.depth);
#define VKV_OCC_WAVES(G, R, C) hipLaunchKernelGGL((k_occupancy_map_waves<G, R, C>), wgrid, dim3(256), 0, s, d_vol, d_grad, d_bits, d_map, W, H, D, mw, mh, bx, by, bz, spans_x, cyw)
#define VKV_OCC_WAVES_G(G)                                                                                                                             \
	do                                                                                                                                                 \
	{                                                                                                                                                  \
		if (crb == 8) VKV_OCC_WAVES(G, 8, 8); else if (crb == 4) VKV_OCC_WAVES(G, 8, 4); else if (crb == 2) VKV_OCC_WAVES(G, 8, 2);                     \
		else if (rows == 8) VKV_OCC_WAVES(G, 8, 1); else if (rows == 9) VKV_OCC_WAVES(G, 9, 1); else if (rows == 10) VKV_OCC_WAVES(G, 10, 1);           \
		else VKV_OCC_WAVES(G, 12, 1);                                                                                                                  \
	} while (0)
			if (precomputed)
				VKV_OCC_WAVES_G(1);
			else
				VKV_OCC_WAVES_G(0);
#undef VKV_OCC_WAVES_G
#undef VKV_OCC_WAVES
			return check_launch(ctx, "occupancy_map");
		}
	}
	if (!tf->use_gradient)
		hipLaunchKernelGGL(k_occupancy_map<0>, grid, dim3(256), 0, s, d_vol, d_grad, d_bits, d_map, W, H, D, mw, mh, md, bx, by,
		                   bz, tf->grad_magnitude_modifier, blocks_x, 0, 0, 0, mw);
	else if (d_grad)
		hipLaunchKernelGGL(k_occupancy_map<1>, grid, dim3(256), 0, s, d_vol, d_grad, d_bits, d_map, W, H, D, mw, mh, md, bx, by,
		                   bz, tf->grad_magnitude_modifier, blocks_x, 0, 0, 0, mw);
	else
		hipLaunchKernelGGL(k_occupancy_map<2>, grid, dim3(256), 0, s, d_vol, d_grad, d_bits, d_map, W, H, D, mw, mh, md, bx, by,
		                   bz, tf->grad_magnitude_modifier, blocks_x, 0, 0, 0, mw);
	return check_launch(ctx, "occupancy_map");
}

// The cells [c0, c1) per axis of the map (a region update's), every one of them written, from the bit table already in d_bits.
// from_distance: d_map holds a transform of the occupancy, which is first turned back into it.
int launch_occupancy_map_cells(vkv_ctx *ctx, const uint8_t *d_vol, const uint8_t *d_grad, const VkvTransferFunctionUniform *tf, VkvExtent3D e,
                               uint8_t *d_map, VkvExtent3D me, const uint32_t c0[3], const uint32_t c1[3], bool from_distance, hipStream_t s,
                               uint32_t *d_bits)
{
	if (from_distance)
	{
		const size_t n_cells = (size_t) me.width * me.height * me.depth;
		const size_t blocks  = std::min<size_t>(std::max<size_t>(1, (n_cells / 16 + 255) / 256), 4096);
		hipLaunchKernelGGL(k_occupancy_of_distance, dim3((uint32_t) blocks), dim3(256), 0, s, d_map, n_cells);
	}
	// src/compute_distance_map.cpp:110-113
	const int bx = (int) block_of(e.width, me.width), by = (int) block_of(e.height, me.height), bz = (int) block_of(e.depth, me.depth);
	const int      cpb      = 256 / bx > 0 ? 256 / bx : 1;
	const uint32_t blocks_x = (c1[0] - c0[0] + cpb - 1) / cpb;
	const dim3     grid(blocks_x * (c1[1] - c0[1]), c1[2] - c0[2]);
#define VKV_OCC_BOX(G_)                                                                                                                                  \
	hipLaunchKernelGGL(k_occupancy_map<G_>, grid, dim3(256), 0, s, d_vol, d_grad, d_bits, d_map, (int) e.width, (int) e.height, (int) e.depth,            \
	                   (int) me.width, (int) me.height, (int) me.depth, bx, by, bz, tf->grad_magnitude_modifier, blocks_x, (int) c0[0], (int) c0[1],   \
	                   (int) c0[2], (int) c1[0])
	if (!tf->use_gradient)
		VKV_OCC_BOX(0);
	else if (d_grad)
		VKV_OCC_BOX(1);
	else
		VKV_OCC_BOX(2);
#undef VKV_OCC_BOX
	return check_launch(ctx, "update_volume_region: occupancy");
}

// the bit table and its column mask, as launch_occupancy_map makes them for itself unless bits_ready
int launch_tf_bits_columns(vkv_ctx *ctx, const uint8_t *d_tf, uint32_t *d_bits, hipStream_t s)
{
	hipLaunchKernelGGL(k_tf_bits, dim3(8), dim3(256), 0, s, d_tf, d_bits);
	hipLaunchKernelGGL(k_tf_columns, dim3(1), dim3(256), 0, s, d_bits);
	return check_launch(ctx, "update_volume_region: bit table");
}

// the occupancy bit table of an RGBA8 texture (k_tf_bits alone: vkv_occupancy_map_from_summary has no use for the column mask)
int launch_tf_bits(vkv_ctx *ctx, const uint8_t *d_tf, uint32_t *d_bits, hipStream_t s)
{
	hipLaunchKernelGGL(k_tf_bits, dim3(8), dim3(256), 0, s, d_tf, d_bits);
	return check_launch(ctx, "transfer_function_bits");
}

// what the voxel count can take: its groups of four rows are counted in 32 bits
bool count_launch_ok(VkvExtent3D e) { return ((uint64_t) e.height * e.depth + 3) / 4 <= 0xffffffffull; }

// d_bits: the bit table in the stream's scratch block (the caller holds its lock)
int launch_occupied_voxel_count(vkv_ctx *ctx, const uint8_t *d_vol, const uint8_t *d_grad, const VkvTransferFunctionUniform *tf, VkvExtent3D e,
                                uint64_t *d_count, hipStream_t s, uint32_t *d_bits)
{
	if (!count_launch_ok(e))
		return set_error(ctx, VKV_E_UNSUPPORTED, "occupied_voxel_count: volume too large");
	hipLaunchKernelGGL(k_tf_bits_analytic, dim3(8), dim3(256), 0, s, d_bits, tf->intensity_min, tf->intensity_range_inv, tf->gradient_min,
	                   tf->gradient_range_inv);
	const hipError_t me = hipMemsetAsync(d_count, 0, sizeof(uint64_t), s);
	if (me != hipSuccess)
		return set_error(ctx, (int) me, "occupied_voxel_count: %s", hipGetErrorString(me));
	// four voxels per lane for every width >= 4 and every alignment (row_dword); the byte path only for the on-the-fly gradient and tiny rows
	const bool     dwords       = e.width >= 4 && (!tf->use_gradient || d_grad);
	const bool     aligned      = (e.width & 3u) == 0 && ((((uintptr_t) d_vol) | ((uintptr_t) d_grad)) & 3u) == 0;
	const uint32_t blocks_x     = dwords ? ((e.width + 3) / 4 + 63) / 64 : (e.width + 63) / 64;
	const uint64_t n_row_groups = ((uint64_t) e.height * e.depth + 3) / 4;
	// ~8 workgroups per CU, grid-stride over the row groups: one atomic per workgroup, few thousand in total
	const uint32_t groups = (uint32_t) (n_row_groups < 2048 / blocks_x + 1 ? n_row_groups : 2048 / blocks_x + 1);
	const dim3     grid(blocks_x * groups);
	unsigned long long *total = reinterpret_cast<unsigned long long *>(d_count);
	const int W = (int) e.width, H = (int) e.height, D = (int) e.depth;
#define VKV_COUNT(G, DW)                                                                                                                                  \
	hipLaunchKernelGGL((k_occupied_voxel_count<G, DW>), grid, dim3(256), 0, s, d_vol, d_grad, d_bits, total, W, H, D, tf->grad_magnitude_modifier,        \
	                   tf->intensity_min, tf->intensity_range_inv, tf->gradient_min, tf->gradient_range_inv, blocks_x, (uint32_t) n_row_groups)
	if (!tf->use_gradient)
	{
		if (dwords && aligned) VKV_COUNT(0, 1); else if (dwords) VKV_COUNT(0, 2); else VKV_COUNT(0, 0);
	}
	else if (d_grad)
	{
		if (dwords && aligned) VKV_COUNT(1, 1); else if (dwords) VKV_COUNT(1, 2); else VKV_COUNT(1, 0);
	}
	else
		VKV_COUNT(2, 0);
#undef VKV_COUNT
	return check_launch(ctx, "occupied_voxel_count");
}

}        // namespace vkv
