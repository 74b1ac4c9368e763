/* SPDX-License-Identifier: BSD-3-Clause
 *
 * Dense per-queue frame batches on the device (include/odpg_gather.h): the
 * frames of a range of delivery buckets written back to back in delivery
 * order, the batch form of the packet move in _odp_cls_enq()
 * (odp_classification_internal.h:139-225).
 *
 * Every kernel reads the range from `offsets` itself (n = e - s positions,
 * odpg_gather.h "Positions"); the grid is sized from src->num on the host and
 * a workgroup whose tile of GTH_TILE = 1024 positions lies beyond n exits
 * after those two loads. The stream order between launches is the only
 * dependency between workgroups (no look-back, flags or grid sync).
 *
 * The unit of all copying is 16 bytes, one global load and one global store
 * of a lane. Frames start on a unit boundary on both sides (odpg_desc_t
 * offsets are multiples of 16, the gathered ones are sums of align16(len)).
 *
 * Fixed stride, one launch (gth_fixed): a tile's destination is the
 * contiguous cnt * stride bytes at j0 * stride. Lane l of step k owns unit
 * u = k * 256 + l of it: frame u / (stride / 16), unit u % (stride / 16);
 * the source frame comes from the tile's `order` entries staged in LDS
 * (read once, coalesced). A lane issues GTH_DEPTH = 4 independent loads, then
 * their 4 stores. stride == 64 is a specialisation with the divide folded
 * into shifts; there a wave moves 16 frames per step. words / desc are
 * written per position by consecutive lanes while `order` is staged.
 *
 * Descriptors, three launches:
 *   gth_units  a workgroup per tile: source {offset, len} of each position
 *              through order -> desc, stored by position in the plan's `pos`
 *              (coalesced 8 B per lane; the copy pass does not chase desc
 *              through order again), and the tile's unit count
 *              sum(align16(len) / 16) into tsum[tile] (64-bit: len is any u32)
 *   gth_scan   one workgroup: exclusive scan of tsum over the live tiles in
 *              place; total = {n, 0, 16 * sum}
 *   gth_copy   a workgroup per tile: pos[] of the tile into LDS, exclusive
 *              scan of the unit counts into start[0 .. 1024] (tile-relative,
 *              u32, saturating: a value that large lies past any capacity);
 *              desc / words per position; then the tile's contiguous
 *              destination range one unit per lane: lane l of step k owns
 *              unit u = k * 256 + l and finds its frame f, start[f] <= u <
 *              start[f + 1], by a binary search of start[] that begins at the
 *              frame it held in the step before (u only grows). It loads
 *              16 B from frames + off[f] + 16 (u - start[f]), zeroes the bytes
 *              past len in a frame's last unit and stores to unit G + u, G
 *              the tile's base from gth_scan. Stores are perfectly coalesced,
 *              loads are coalesced within a frame, and every lane moves the
 *              same number of bytes whatever the length mix: the reason to
 *              split by destination unit and not by packet (1518 B next to
 *              64 B is 95 units next to 4).
 *              Capacity: position p is copied iff G + start[p + 1] <=
 *              capacity / 16. That holds for a prefix of nc positions, the
 *              copy loop runs over start[nc] units, and nc is added to
 *              total->copied (one integer atomic per tile).
 *
 * LDS, bytes: gth_copy start 4100 + off 4096 + len 4096 + scan 32 + nc 4 =
 * 12328; gth_fixed 4096; gth_units 32; gth_scan 128. Registers and scratch:
 * DESIGN "Dense queue batches".
 */
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>

#include "gather.h"

namespace {

constexpr uint32_t T = GTH_TILE;
constexpr uint32_t WG = 256;                /* lanes of a tile's workgroup */
constexpr uint32_t WAVES = WG / 64;
constexpr uint32_t PPL = T / WG;            /* positions per lane */
constexpr uint32_t DEPTH = 4;               /* 16-byte loads a lane keeps in flight */
constexpr uint32_t SCAN_WG = 1024;
constexpr uint32_t SAT = 0x7FFFFFFFu;       /* units: beyond capacity / 16 <= 2^28 */

static_assert(PPL == 4 && T % WG == 0, "tile shape");

typedef odpg_gather_args Args;

struct Range {
	uint32_t s, n;
};

__device__ __forceinline__ Range range_of(const Args &a)
{
	const uint32_t e = min(a.offsets[a.b_last], a.src.num);
	const uint32_t s = min(a.offsets[a.b_first], e);

	return {s, e - s};
}

__device__ __forceinline__ uint64_t units_of(uint32_t len)
{
	return ((uint64_t)len + 15u) >> 4;
}

/* exclusive prefix of v over the workgroup's lanes (ws: one word per wave);
 * *total: the sum over all of them */
template <uint32_t NW>
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t *ws, uint64_t *total)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint64_t inc = v;

	for (uint32_t off = 1; off < 64u; off <<= 1) {
		const uint64_t t = __shfl_up(inc, off);

		if (lane >= off)
			inc += t;
	}
	if (lane == 63u)
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

/* the low `nb` bytes of w (nb <= 0: none, nb >= 4: all) */
__device__ __forceinline__ uint32_t keep_bytes(uint32_t w, int32_t nb)
{
	return nb >= 4 ? w : nb <= 0 ? 0u : w & ((1u << (8 * nb)) - 1u);
}

/* ---- fixed stride ---------------------------------------------------------- */
template <uint32_t STRIDE>   /* 64, or 0: any multiple of 16 */
__global__ __launch_bounds__(WG) void gth_fixed(Args a)
{
	__shared__ uint32_t s_ord[T];
	const uint32_t tid = threadIdx.x, j0 = blockIdx.x * T;
	const Range r = range_of(a);
	const uint32_t stride = STRIDE ? STRIDE : a.src.stride, upl = stride >> 4;
	/* frames that fit: capacity <= 2^32 and stride >= 16 */
	const uint32_t fit = (uint32_t)min((uint64_t)r.n, a.dst.capacity / stride);

	if (blockIdx.x == 0 && tid == 0) {
		a.dst.total->num = r.n;
		a.dst.total->copied = fit;
		a.dst.total->bytes = (uint64_t)r.n * stride;
	}
	if (j0 >= r.n)
		return;
	const uint32_t cnt = min(T, r.n - j0);
	const uint32_t ncopy = fit > j0 ? min(cnt, fit - j0) : 0u;

	for (uint32_t p = tid; p < cnt; p += WG) {
		const uint32_t i = a.order[r.s + j0 + p];

		s_ord[p] = i;
		if (a.dst.words)
			a.dst.words[j0 + p] = i < a.src.num ? a.src.words[i] : 0u;
		if (a.dst.desc) {
			/* a copied frame ends at or below 2^32 */
			const uint32_t off = (j0 + p) * stride;

			((uint2 *)a.dst.desc)[j0 + p] = p < ncopy ? make_uint2(off, stride)
								  : make_uint2(0u, 0u);
		}
	}
	__syncthreads();
	/* ncopy * stride <= capacity: at most 2^28 units */
	const uint32_t nu = ncopy * upl;
	uint4 *dst = (uint4 *)(a.dst.frames + (uint64_t)j0 * stride);

	for (uint32_t u0 = tid; u0 < nu; u0 += DEPTH * WG) {
		uint4 v[DEPTH];

#pragma unroll
		for (uint32_t k = 0; k < DEPTH; k++) {
			const uint32_t u = u0 + k * WG;

			v[k] = make_uint4(0u, 0u, 0u, 0u);
			if (u < nu) {
				const uint32_t p = u / upl;   /* a shift when STRIDE is 64 */
				const uint32_t i = s_ord[p];

				if (i < a.src.num)
					v[k] = *(const uint4 *)(a.src.frames + (uint64_t)i * stride +
								16u * (u - p * upl));
			}
		}
#pragma unroll
		for (uint32_t k = 0; k < DEPTH; k++)
			if (u0 + k * WG < nu)
				dst[u0 + k * WG] = v[k];
	}
}

/* ---- descriptors, launch 1: source descriptors by position, tile sums ------ */
__global__ __launch_bounds__(WG) void gth_units(Args a)
{
	__shared__ uint64_t s_ws[WAVES];
	const uint32_t tid = threadIdx.x, j0 = blockIdx.x * T;
	const Range r = range_of(a);
	uint32_t idx[PPL];
	uint2 d[PPL];
	uint64_t sum = 0;

	if (j0 >= r.n)
		return;
#pragma unroll
	for (uint32_t k = 0; k < PPL; k++) {
		const uint32_t j = j0 + k * WG + tid;

		idx[k] = j < r.n ? a.order[r.s + j] : 0xFFFFFFFFu;
	}
#pragma unroll
	for (uint32_t k = 0; k < PPL; k++) {
		d[k] = make_uint2(0u, 0u);
		if (idx[k] < a.src.num)
			d[k] = ((const uint2 *)a.src.desc)[idx[k]];
	}
#pragma unroll
	for (uint32_t k = 0; k < PPL; k++) {
		const uint32_t j = j0 + k * WG + tid;

		if (j < r.n)
			((uint2 *)a.pos)[j] = d[k];
		sum += units_of(d[k].y);
	}
	for (uint32_t off = 32; off; off >>= 1)
		sum += __shfl_xor(sum, off);
	if ((tid & 63u) == 0)
		s_ws[tid >> 6] = sum;
	__syncthreads();
	if (tid == 0) {
		sum = 0;
		for (uint32_t w = 0; w < WAVES; w++)
			sum += s_ws[w];
		a.tsum[blockIdx.x] = sum;
	}
}

/* ---- launch 2: tile sums -> tile bases, total ------------------------------ */
__global__ __launch_bounds__(SCAN_WG) void gth_scan(Args a)
{
	__shared__ uint64_t s_ws[SCAN_WG / 64];
	const uint32_t tid = threadIdx.x;
	const Range r = range_of(a);
	const uint32_t ntiles = r.n / T + (r.n % T != 0);
	uint64_t carry = 0;

	for (uint32_t base = 0; base < ntiles; base += SCAN_WG) {
		const uint32_t t = base + tid;
		const uint64_t v = t < ntiles ? a.tsum[t] : 0u;
		uint64_t all;
		const uint64_t before = block_excl_scan<SCAN_WG / 64>(v, s_ws, &all);

		if (t < ntiles)
			a.tsum[t] = carry + before;
		carry += all;
	}
	if (tid == 0) {
		a.dst.total->num = r.n;
		a.dst.total->copied = 0;     /* gth_copy adds each tile's share */
		a.dst.total->bytes = carry << 4;
	}
}

/* ---- launch 3: copy, one unit per lane ------------------------------------- */
__global__ __launch_bounds__(WG) void gth_copy(Args a)
{
	__shared__ uint32_t s_start[T + 1];
	__shared__ uint32_t s_off[T];
	__shared__ uint32_t s_len[T];
	__shared__ uint64_t s_ws[WAVES];
	__shared__ uint32_t s_nc;
	const uint32_t tid = threadIdx.x, j0 = blockIdx.x * T;
	const Range r = range_of(a);

	if (j0 >= r.n)
		return;
	const uint32_t cnt = min(T, r.n - j0);
	const uint64_t G = a.tsum[blockIdx.x], capu = a.dst.capacity >> 4;
	uint2 d[PPL];
	uint64_t sum = 0, all;

	/* lane-blocked: positions [4 tid, 4 tid + 4), 32 B per lane */
	if (cnt == T) {
		const uint4 *q = (const uint4 *)(a.pos + j0) + 2u * tid;
		const uint4 x = q[0], y = q[1];

		d[0] = make_uint2(x.x, x.y);
		d[1] = make_uint2(x.z, x.w);
		d[2] = make_uint2(y.x, y.y);
		d[3] = make_uint2(y.z, y.w);
	} else {
#pragma unroll
		for (uint32_t k = 0; k < PPL; k++) {
			const uint32_t p = PPL * tid + k;

			d[k] = p < cnt ? ((const uint2 *)a.pos)[j0 + p] : make_uint2(0u, 0u);
		}
	}
#pragma unroll
	for (uint32_t k = 0; k < PPL; k++)
		sum += units_of(d[k].y);
	if (tid == 0)
		s_nc = 0;
	uint64_t run = block_excl_scan<WAVES>(sum, s_ws, &all);

	/* positions past cnt have no units: start[cnt .. T] = the tile's total */
#pragma unroll
	for (uint32_t k = 0; k < PPL; k++) {
		const uint32_t p = PPL * tid + k;

		s_start[p] = (uint32_t)min(run, (uint64_t)SAT);
		s_off[p] = d[k].x;
		s_len[p] = d[k].y;
		run += units_of(d[k].y);
	}
	if (tid == WG - 1u)
		s_start[T] = (uint32_t)min(all, (uint64_t)SAT);
	__syncthreads();

	for (uint32_t p = tid; p < cnt; p += WG) {
		const uint32_t st = s_start[p];
		const bool fits = G + s_start[p + 1u] <= capu;

		/* a copied frame ends at or below 2^32 (a zero-length frame at
		 * exactly 2^32 gets offset 0) */
		((uint2 *)a.dst.desc)[j0 + p] = fits ? make_uint2((uint32_t)((G + st) << 4), s_len[p])
						     : make_uint2(0u, 0u);
		if (a.dst.words) {
			const uint32_t i = a.order[r.s + j0 + p];

			a.dst.words[j0 + p] = i < a.src.num ? a.src.words[i] : 0u;
		}
		/* ends are monotone: the last position that fits ends the prefix */
		if (fits && (p + 1u == cnt || G + s_start[p + 2u] > capu))
			s_nc = p + 1u;
	}
	__syncthreads();
	const uint32_t nc = s_nc;
	const uint32_t nu = s_start[nc];          /* <= capu - G <= 2^28 */

	if (tid == 0 && nc)
		atomicAdd(&a.dst.total->copied, nc);
	uint4 *dst = (uint4 *)a.dst.frames + G;
	uint32_t f = 0;

	for (uint32_t u0 = tid; u0 < nu; u0 += DEPTH * WG) {
		uint64_t src[DEPTH];     /* byte offsets into src.frames */
		uint32_t left[DEPTH];
		uint4 v[DEPTH];

		/* the searches first, then the loads back to back, then masks and
		 * stores: a mask right behind its load would wait for it and leave
		 * one load in flight per lane */
#pragma unroll
		for (uint32_t k = 0; k < DEPTH; k++) {
			const uint32_t u = u0 + k * WG;

			if (u < nu) {
				/* the first frame from f on that ends beyond u: one
				 * exists below nc because u < start[nc] */
				uint32_t hi = nc - 1u;

				while (f < hi) {
					const uint32_t mid = (f + hi) >> 1;

					if (s_start[mid + 1u] > u)
						hi = mid;
					else
						f = mid + 1u;
				}
				const uint32_t q = u - s_start[f];

				left[k] = s_len[f] - 16u * q;   /* >= 1 */
				src[k] = s_off[f] + 16ull * q;
			}
		}
#pragma unroll
		for (uint32_t k = 0; k < DEPTH; k++)
			if (u0 + k * WG < nu)
				v[k] = *(const uint4 *)(a.src.frames + src[k]);
#pragma unroll
		for (uint32_t k = 0; k < DEPTH; k++) {
			if (u0 + k * WG < nu) {
				if (left[k] < 16u) {
					const int32_t nb = (int32_t)left[k];

					v[k].x = keep_bytes(v[k].x, nb);
					v[k].y = keep_bytes(v[k].y, nb - 4);
					v[k].z = keep_bytes(v[k].z, nb - 8);
					v[k].w = keep_bytes(v[k].w, nb - 12);
				}
				dst[u0 + k * WG] = v[k];
			}
		}
	}
}

} /* namespace */

extern "C" int odpg_launch_gather(const odpg_gather_args *a, hipStream_t s)
{
	/* at least one workgroup: it writes `total` when the batch is empty */
	const uint32_t ntiles = a->src.num ? (a->src.num - 1u) / T + 1u : 1u;

	if (!a->src.desc) {
		if (a->src.stride == 64u)
			hipLaunchKernelGGL(gth_fixed<64u>, dim3(ntiles), dim3(WG), 0, s, *a);
		else
			hipLaunchKernelGGL(gth_fixed<0u>, dim3(ntiles), dim3(WG), 0, s, *a);
		return hipGetLastError() == hipSuccess ? 0 : -EIO;
	}
	hipLaunchKernelGGL(gth_units, dim3(ntiles), dim3(WG), 0, s, *a);
	hipLaunchKernelGGL(gth_scan, dim3(1), dim3(SCAN_WG), 0, s, *a);
	hipLaunchKernelGGL(gth_copy, dim3(ntiles), dim3(WG), 0, s, *a);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
