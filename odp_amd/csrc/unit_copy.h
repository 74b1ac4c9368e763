/* SPDX-License-Identifier: BSD-3-Clause
 *
 * Device helpers shared by the kernels that move frames in 16-byte units
 * (lso.hip, reass.hip): the byte funnel that builds a unit from the two
 * aligned units around an arbitrary source byte, tail masks, wave and
 * workgroup scans and the search from a unit to the frame that holds it.
 */
#ifndef ODPG_UNIT_COPY_H_
#define ODPG_UNIT_COPY_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint32_t units_of(uint32_t len)
{
	return (uint32_t)(((uint64_t)len + 15u) >> 4);
}

/* the low `nb` bytes of w (nb <= 0: none, nb >= 4: all) */
__device__ __forceinline__ uint32_t keep_bytes(uint32_t w, int32_t nb)
{
	return nb >= 4 ? w : nb <= 0 ? 0u : w & ((1u << (8 * nb)) - 1u);
}

__device__ __forceinline__ uint4 keep_unit(uint4 v, int32_t nb)
{
	return make_uint4(keep_bytes(v.x, nb), keep_bytes(v.y, nb - 4), keep_bytes(v.z, nb - 8),
			  keep_bytes(v.w, nb - 12));
}

/* bytes [sh, sh + 16) of the 32 bytes lo | hi, sh in [0, 16) */
__device__ __forceinline__ uint4 funnel(uint4 lo, uint4 hi, uint32_t sh)
{
	const bool s8 = sh & 8u, s4 = sh & 4u;
	uint32_t w0 = s8 ? lo.z : lo.x, w1 = s8 ? lo.w : lo.y, w2 = s8 ? hi.x : lo.z;
	uint32_t w3 = s8 ? hi.y : lo.w, w4 = s8 ? hi.z : hi.x, w5 = s8 ? hi.w : hi.y;

	w0 = s4 ? w1 : w0;
	w1 = s4 ? w2 : w1;
	w2 = s4 ? w3 : w2;
	w3 = s4 ? w4 : w3;
	w4 = s4 ? w5 : w4;
	const uint32_t b = sh & 3u;

	return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, b), __builtin_amdgcn_alignbyte(w2, w1, b),
			  __builtin_amdgcn_alignbyte(w3, w2, b), __builtin_amdgcn_alignbyte(w4, w3, b));
}

/* inclusive prefix over the 64 lanes of a wave */
template <typename V>
__device__ __forceinline__ V wave_incl_scan(V v)
{
	const uint32_t lane = threadIdx.x & 63u;

	for (uint32_t off = 1; off < 64u; off <<= 1) {
		const V t = __shfl_up(v, off);

		if (lane >= off)
			v += t;
	}
	return v;
}

/* exclusive prefix of v over the workgroup's lanes (ws: one word per wave);
 * *total: the sum over all of them */
template <uint32_t NW>
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t *ws, uint64_t *total)
{
	const uint32_t wave = threadIdx.x >> 6;
	const uint64_t inc = wave_incl_scan(v);

	if ((threadIdx.x & 63u) == 63u)
		ws[wave] = inc;
	__syncthreads();
	uint64_t base = 0, all = 0;

	for (uint32_t w = 0; w < NW; w++) {
		const uint64_t c = ws[w];

		base += w < wave ? c : 0u;
		all += c;
	}
	__syncthreads();
	*total = all;
	return base + inc - v;
}

/* the first f in [f, last] with arr[f + 1] > x; the caller knows one exists */
__device__ __forceinline__ uint32_t find_from(const uint32_t *arr, uint32_t f, uint32_t x,
					      uint32_t last)
{
	uint32_t hi = last;

	while (f < hi) {
		const uint32_t mid = (f + hi) >> 1;

		if (arr[mid + 1u] > x)
			hi = mid;
		else
			f = mid + 1u;
	}
	return f;
}

#endif
