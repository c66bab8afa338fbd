// tf_tables.hip — what the integrator and the map passes read of a transfer function, made on the device: the alpha > 0 bit table, the
// separable alpha tables and their flag word from an RGBA8 texture (k_tf_tables_init + k_tf_tables: vkv_transfer_function_tables, which checks
// the separable claim against every texel), or the texture itself with all of these from the uniform's fields in one launch (k_tf_build:
// vkv_transfer_function_texture_device, vkv_update_transfer_function).  The occupancy pass's bit table of a texture is k_tf_bits in occupancy.hip.
#include "launchers.hpp"

namespace vkv
{

// Separable alpha tables of the reference's transfer function (src/volume_component.cpp:246-261) from the uniform's fields, and
// the flag word.  has_tf == 0: no claim, flag clear.
__global__ void __launch_bounds__(256) k_tf_tables_init(uint32_t *__restrict__ tables, int has_tf, float imin, float iinv, float gmin, float ginv, int use_gradient)
{
	const int   i = threadIdx.x;
	const float x = (float) i / 255.0f;
	float       ai = (x - imin) * iinv, ag = 1.0f;
	ai = (ai < 0.0f) ? 0.0f : ai, ai = (1.0f < ai) ? 1.0f : ai;        // std::max / std::min as the host writes them
	if (use_gradient)
	{
		ag = (x - gmin) * ginv;
		ag = (ag < 0.0f) ? 0.0f : ag, ag = (1.0f < ag) ? 1.0f : ag;
	}
	tables[kTfAiWord + i] = __float_as_uint(ai);
	tables[kTfAgWord + i] = __float_as_uint(ag);
	if (i < 4)
		tables[kTfFlagWord + i] = (i == 0 && has_tf) ? kTfFlagSeparable : 0u;
}

// alpha > 0 bit table + the check of the separable claim against every texel (clears the flag on the first mismatch)
__global__ void __launch_bounds__(256) k_tf_tables(const uint8_t *__restrict__ tf_rgba8, uint32_t *__restrict__ tables, int has_tf)
{
	const uint32_t w = blockIdx.x * 256 + threadIdx.x;        // 2048 words of 32 texels
	if (w >= 2048)
		return;
	uint32_t v = 0;
	bool     ok = true;
	for (int i = 0; i < 32; ++i)
	{
		const uint32_t t     = w * 32 + i;
		const uint32_t texel = reinterpret_cast<const uint32_t *>(tf_rgba8)[t];
		v |= ((texel >> 24) > 0 ? 1u : 0u) << i;
		if (has_tf)
		{
			const uint32_t b = tf_separable_alpha(__uint_as_float(tables[kTfAiWord + (t & 255u)]), __uint_as_float(tables[kTfAgWord + (t >> 8)]));
			ok               = ok && texel == b * 0x01010101u;
		}
	}
	tables[w] = v;
	if (has_tf && !ok)
		atomicAnd(&tables[kTfFlagWord], ~kTfFlagSeparable);
}

int launch_tf_tables(vkv_ctx *ctx, const uint8_t *d_tf, const VkvTransferFunctionUniform *tf, uint32_t *d_tables, hipStream_t s)
{
	const int has_tf = tf != nullptr;
	hipLaunchKernelGGL(k_tf_tables_init, dim3(1), dim3(256), 0, s, d_tables, has_tf, has_tf ? tf->intensity_min : 0.0f, has_tf ? tf->intensity_range_inv : 0.0f,
	                   has_tf ? tf->gradient_min : 0.0f, has_tf ? tf->gradient_range_inv : 0.0f, has_tf ? (int) (tf->use_gradient != 0) : 0);
	hipLaunchKernelGGL(k_tf_tables, dim3(8), dim3(256), 0, s, d_tf, d_tables, has_tf);
	return check_launch(ctx, "transfer_function_tables");
}

// The whole transfer function of the reference (src/volume_component.cpp:242-278) from the uniform's fields, without a host loop or an
// upload: the RGBA8 texture, the integrator's tables (what k_tf_tables_init + k_tf_tables make of that texture) and, when `bits` is given,
// the occupancy pass's bit table + column mask (what k_tf_bits + k_tf_columns leave in the stream's scratch block).  One workgroup per
// gradient row, one lane per intensity column: one dword store per texel, the row's alpha > 0 bits out of one ballot per wave.
// The texel is the host's expression (vkv_transfer_function_texture): comparison clamps as std::max / std::min write them, (a_i * a_g) * 255
// as two multiplies, truncation.  A NaN product - intensity_max == intensity_min gives one at the column where i / 255 == intensity_min -
// stores 0, the byte (uint8) NaN gives on x86-64.  The separable flag holds by construction.
__device__ __forceinline__ float tf_axis_alpha(uint32_t i, float lo, float inv)
{
	const float x = (float) i / 255.0f;
	float       a = (x - lo) * inv;
	a = (a < 0.0f) ? 0.0f : a, a = (1.0f < a) ? 1.0f : a;        // std::max / std::min as the host writes them
	return a;
}
__device__ __forceinline__ uint32_t tf_texel_alpha(float ai, float ag)
{
	const float p = (ai * ag) * 255.0f;        // in [0, 255] or NaN: the host's clamp to [0, 255] changes nothing else
	return p == p ? (uint32_t) p : 0u;
}

__global__ void __launch_bounds__(256) k_tf_build(uint32_t *__restrict__ tex, uint32_t *__restrict__ tables, uint32_t *__restrict__ bits, float imin,
                                                  float iinv, float gmin, float ginv, int use_gradient)
{
	__shared__ float s_max[4];
	const uint32_t   i  = threadIdx.x, g = blockIdx.x;        // intensity column, gradient row
	const float      ai = tf_axis_alpha(i, imin, iinv);
	const float      ag = use_gradient ? tf_axis_alpha(g, gmin, ginv) : 1.0f;
	const uint32_t   b  = tf_texel_alpha(ai, ag);
	tex[g * 256u + i]   = b * 0x01010101u;
	const unsigned long long m = __builtin_amdgcn_ballot_w64(b != 0u);
	if ((i & 63u) == 0u)
	{
		const uint32_t w = g * 8u + (i >> 5);
		tables[w] = (uint32_t) m, tables[w + 1u] = (uint32_t) (m >> 32);
		if (bits)
			bits[w] = (uint32_t) m, bits[w + 1u] = (uint32_t) (m >> 32);
	}
	if (g != 0u)
		return;
	// workgroup 0: the separable tables (lane i also holds row i's a_g), the flag words and the column mask.  Column i has an occupied texel iff
	// (uint8) (a_i[i] * max_g a_g * 255) > 0: the product is monotone in a_g >= 0, and a row whose a_g is NaN has none (it counts as 0)
	const float agi = use_gradient ? tf_axis_alpha(i, gmin, ginv) : 1.0f;
	tables[kTfAiWord + i] = __float_as_uint(ai);
	tables[kTfAgWord + i] = __float_as_uint(agi);
	if (i < 4u)
		tables[kTfFlagWord + i] = i == 0u ? kTfFlagSeparable : 0u;
	if (!bits)
		return;
	float mx = agi == agi ? agi : 0.0f;
	for (int o = 32; o > 0; o >>= 1)
		mx = g_max(mx, __shfl_xor(mx, o));
	if ((i & 63u) == 0u)
		s_max[i >> 6] = mx;
	__syncthreads();
	mx = g_max(g_max(s_max[0], s_max[1]), g_max(s_max[2], s_max[3]));
	const unsigned long long c = __builtin_amdgcn_ballot_w64(tf_texel_alpha(ai, mx) != 0u);
	if ((i & 63u) == 0u)
		bits[2048u + (i >> 5)] = (uint32_t) c, bits[2048u + (i >> 5) + 1u] = (uint32_t) (c >> 32);
}

int launch_tf_build(vkv_ctx *ctx, const VkvTransferFunctionUniform *tf, uint8_t *d_tf, uint32_t *d_tables, uint32_t *d_bits, hipStream_t s)
{
	hipLaunchKernelGGL(k_tf_build, dim3(256), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d_tf), d_tables, d_bits, tf->intensity_min,
	                   tf->intensity_range_inv, tf->gradient_min, tf->gradient_range_inv, (int) (tf->use_gradient != 0));
	return check_launch(ctx, "transfer_function_texture_device");
}

}        // namespace vkv
