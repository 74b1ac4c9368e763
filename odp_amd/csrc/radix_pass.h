/* SPDX-License-Identifier: BSD-3-Clause
 *
 * The stable least-significant-digit-first radix partition of packet indices
 * by a small integer key, shared by deliver.hip (key: the delivery bucket of
 * a verdict word) and switch.hip (key: a frame's MAC-table slot). Each file
 * that includes this header gets its own copy of the kernels, instantiated
 * for its Source:
 *
 *   struct Source {
 *       const uint32_t *src;   // pass 0: one word per packet
 *       uint32_t num;
 *       __device__ uint32_t key(uint32_t word) const;   // < nbuckets
 *   };
 *
 * Passes. The key has rp_ws::key_bits bits. Up to DLV_DIGIT_BITS = 11 bits
 * it is one digit and one pass. Wider keys, up to 22 bits, are split in two
 * digits of half the bits: pass 0 reads the words and writes {key, index}
 * pairs to the pair buffer, pass 1 reads the pairs and writes `order`. A pass
 * only spends ballots, counters and histogram columns on the bits its digit
 * has.
 *
 * Per pass three launches on one stream; the order between launches is the
 * only dependency between workgroups (no workgroup waits on another):
 *   dlv_hist     one workgroup per tile of DLV_TILE = 4096 packets: digit
 *                counts of the tile into hist[tile][digit], and added into
 *                dtotal[digit] (one global atomic per digit present)
 *   dlv_scan     one workgroup per 64 digits: the digits' global base from
 *                dtotal, then the running sum over the tiles, in place:
 *                hist[tile][digit] becomes the position of the tile's first
 *                packet of that digit. In a one-pass plan the digit bases are
 *                `offsets`. In a two-pass plan the bucket counts pass 0's
 *                histogram kernel also made (bcount[B]) are scanned into
 *                `offsets` by one more workgroup of pass 1's launch.
 *   dlv_scatter  one workgroup per tile: ranks its packets and writes them
 *
 * Scatter workgroup: 512 lanes = 8 waves, 8 packets per lane. Wave w owns the
 * tile's packets [512 w, 512 w + 512) as 8 contiguous runs of 64, lane l of
 * run r holding packet 512 w + 64 r + l, so lane order is arrival order.
 *   - Words arrive 16 B per lane (a full tile whose words are 16-byte
 *     aligned; 4 B per lane otherwise) and pass through LDS once to get from
 *     that layout into run order.
 *   - Rank. One __ballot per digit bit leaves each lane the set of lanes of
 *     its run with the same digit; its rank in the wave is the number of
 *     those below it plus the wave's running count of the digit, a 16-bit
 *     LDS counter the lowest peer advances after every lane has read it. No
 *     atomic orders anything.
 *   - The 8 x ndig wave counters are then scanned over the waves per digit,
 *     the tile's digit totals over the digits, and hist[tile][digit] added.
 *   - Packets are placed in LDS in tile-sorted order beside their global
 *     position, then written out by consecutive lanes: a run of packets for
 *     one bucket leaves as one contiguous store.
 * A wave counter holds at most 512 and, after the scan over the waves, at
 * most the 4096 packets of a tile that falls in one bucket: 16 bits suffice.
 *
 * LDS of dlv_scatter (160 KiB per CU on gfx950), bytes:
 *   s_a     4096 x 4   16384   words, then packet indices, staged
 *   s_dst   4096 x 4   16384   global position of each staged packet
 *   s_key   4096 x 4   16384   staged keys (pass 0 of two only)
 *   s_cnt   8 x 2048 x 2  32768   per-wave digit counters (u16)
 *   s_tb    2048 x 4    8192   tile digit totals -> tile-local digit base
 *   s_gb    2048 x 4    8192   hist[tile][digit] - tile-local digit base
 *   s_ws    8 x 4         32   block scan
 *                      ------
 *                      98336   (81952 in a last pass): one workgroup per CU
 * dlv_hist: 2048 x 4 = 8192. dlv_scan: (16 + 1) x 64 x 4 + 64 = 4416.
 */
#ifndef ODPG_RADIX_PASS_H_
#define ODPG_RADIX_PASS_H_

#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>

#include "deliver.h"   /* DLV_TILE, DLV_RADIX, dlv_bits0 */

namespace {
namespace rp {

constexpr uint32_t T = DLV_TILE;
constexpr uint32_t WG = 512;                /* lanes of a hist / scatter workgroup */
constexpr uint32_t WAVES = WG / 64;
constexpr uint32_t IPL = T / WG;            /* packets per lane = runs per wave */
constexpr uint32_t WAVE_PKTS = T / WAVES;
constexpr uint32_t RADIX = DLV_RADIX;
constexpr uint32_t SCAN_WG = 1024;          /* dlv_scan: 64 digits x 16 tile ranges */
constexpr uint32_t SCAN_WAVES = SCAN_WG / 64;

static_assert(RADIX % WG == 0 && T % (4 * WG) == 0 && WAVE_PKTS <= 0xFFFFu && T <= 0xFFFFu,
	      "tile shape");

/* the lanes of `active` whose low `nbits` bits of v equal this lane's */
__device__ __forceinline__ uint64_t match_lanes(uint32_t v, uint32_t nbits, uint64_t active)
{
	uint64_t m = active;

	for (uint32_t b = 0; b < nbits; b++) {
		const bool bit = (v >> b) & 1u;
		const uint64_t set = __ballot(bit);

		m &= bit ? set : ~set;
	}
	return m;
}

/* exclusive prefix of v over the workgroup's lanes (ws: one word per wave) */
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *ws)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t inc = v;

	for (uint32_t off = 1; off < 64u; off <<= 1) {
		const uint32_t t = __shfl_up(inc, off);

		if (lane >= off)
			inc += t;
	}
	if (lane == 63u)
		ws[wave] = inc;
	__syncthreads();
	uint32_t base = 0;

	for (uint32_t w = 0; w < wave; w++)
		base += ws[w];
	__syncthreads();
	return base + inc - v;
}

/* ---- launch 1: digit counts of every tile --------------------------------
 * Counting needs no order, so a lane keeps the words its 16-byte loads gave
 * it. Lanes of a run with the same remaining key (every bit from `shift` up:
 * the same digit, and in pass 0 the same bucket) are counted by the lowest of
 * them with one LDS add, so a tile in one bucket costs 64 adds, not 4096. */
template <class Source, bool WORDS>
__global__ __launch_bounds__(WG) void dlv_hist(Source s, uint32_t shift, uint32_t nbits,
					       uint32_t mbits, uint32_t *hist,
					       uint32_t *dtotal, uint32_t *bcount)
{
	__shared__ uint32_t s_h[RADIX];
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	const uint32_t ndig = 1u << nbits, base = blockIdx.x * T;
	const uint64_t below = (1ull << lane) - 1ull;
	uint32_t key[IPL];
	uint32_t valid = 0;

	for (uint32_t d = tid; d < ndig; d += WG)
		s_h[d] = 0;
	if (WORDS && s.num - base >= T && ((uintptr_t)s.src & 15u) == 0) {
		const uint4 *p = (const uint4 *)(s.src + base);

#pragma unroll
		for (uint32_t k = 0; k < IPL / 4u; k++) {
			const uint4 v = p[k * WG + tid];

			key[4 * k + 0] = s.key(v.x);
			key[4 * k + 1] = s.key(v.y);
			key[4 * k + 2] = s.key(v.z);
			key[4 * k + 3] = s.key(v.w);
		}
		valid = (1u << IPL) - 1u;
	} else {
#pragma unroll
		for (uint32_t r = 0; r < IPL; r++) {
			const uint32_t i = base + r * WG + tid;

			key[r] = 0;
			if (i < s.num) {
				key[r] = WORDS ? s.key(s.src[i])
					       : ((const uint2 *)s.src)[i].x;
				valid |= 1u << r;
			}
		}
	}
	__syncthreads();
#pragma unroll
	for (uint32_t r = 0; r < IPL; r++) {
		const bool ok = (valid >> r) & 1u;
		const uint64_t peers = match_lanes(key[r] >> shift, mbits, __ballot(ok));

		if (ok && !(peers & below)) {
			const uint32_t c = (uint32_t)__popcll(peers);

			atomicAdd(&s_h[(key[r] >> shift) & (ndig - 1u)], c);
			if (bcount)
				atomicAdd(&bcount[key[r]], c);
		}
	}
	__syncthreads();
	for (uint32_t d = tid; d < ndig; d += WG) {
		const uint32_t c = s_h[d];

		hist[(size_t)blockIdx.x * ndig + d] = c;
		if (c)
			atomicAdd(&dtotal[d], c);
	}
}

/* ---- launch 2: scan over (digit, tile) ------------------------------------
 * Workgroup g: digits [64 g, 64 g + 64), lane = digit, wave = one of 16
 * contiguous ranges of the tiles. Workgroup `ngroups` (two-pass plans, last
 * pass): bucket counts -> offsets. */
__global__ __launch_bounds__(SCAN_WG) void dlv_scan(uint32_t *hist, const uint32_t *dtotal,
						    uint32_t ntiles, uint32_t nbits,
						    uint32_t *offsets, uint32_t nbuckets,
						    uint32_t num, uint32_t *bcount,
						    uint32_t ngroups)
{
	__shared__ uint32_t s_part[SCAN_WAVES];
	__shared__ uint32_t s_db[64];
	__shared__ uint32_t s_cs[SCAN_WAVES][64];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint32_t ndig = 1u << nbits;

	if (blockIdx.x == ngroups) {
		/* a contiguous slice of the buckets per lane */
		const uint32_t per = (nbuckets + SCAN_WG - 1u) / SCAN_WG;
		const uint32_t i0 = min(nbuckets, tid * per), i1 = min(nbuckets, i0 + per);
		uint32_t sum = 0;

		for (uint32_t i = i0; i < i1; i++)
			sum += bcount[i];
		uint32_t run = block_excl_scan(sum, s_part);

		for (uint32_t i = i0; i < i1; i++) {
			const uint32_t c = bcount[i];

			offsets[i] = run;
			run += c;
			bcount[i] = 0;
		}
		if (tid == 0)
			offsets[nbuckets] = num;
		return;
	}
	const uint32_t d0 = blockIdx.x * 64u, d = d0 + lane;
	const bool live = d < ndig;
	uint32_t before = 0;

	/* packets of the digits before this group's */
	for (uint32_t i = tid; i < d0; i += SCAN_WG)
		before += dtotal[i];
	for (uint32_t off = 32; off; off >>= 1)
		before += __shfl_xor(before, off);
	if (lane == 0)
		s_part[wave] = before;
	__syncthreads();
	if (wave == 0) {
		const uint32_t v = live ? dtotal[d] : 0u;
		uint32_t inc = v;

		before = 0;
		for (uint32_t w = 0; w < SCAN_WAVES; w++)
			before += s_part[w];
		for (uint32_t off = 1; off < 64u; off <<= 1) {
			const uint32_t t = __shfl_up(inc, off);

			if (lane >= off)
				inc += t;
		}
		s_db[lane] = before + inc - v;
		/* one pass: the digit is the bucket, its base the bucket's offset */
		if (offsets && !bcount) {
			if (live && d <= nbuckets)
				offsets[d] = before + inc - v;
			if (d == 0 && nbuckets == ndig)
				offsets[nbuckets] = num;
		}
	}
	const uint32_t per = (ntiles + SCAN_WAVES - 1u) / SCAN_WAVES;
	const uint32_t t0 = min(ntiles, wave * per), t1 = min(ntiles, t0 + per);
	uint32_t sum = 0;

	if (live) {
#pragma unroll 8
		for (uint32_t t = t0; t < t1; t++)
			sum += hist[(size_t)t * ndig + d];
	}
	s_cs[wave][lane] = sum;
	__syncthreads();
	if (!live)
		return;
	uint32_t run = s_db[lane];

	for (uint32_t w = 0; w < wave; w++)
		run += s_cs[w][lane];
	/* eight loads in flight, then their stores */
	for (uint32_t t = t0; t < t1; t += 8u) {
		uint32_t v[8];

#pragma unroll
		for (uint32_t j = 0; j < 8u; j++)
			v[j] = t + j < t1 ? hist[(size_t)(t + j) * ndig + d] : 0u;
#pragma unroll
		for (uint32_t j = 0; j < 8u; j++) {
			if (t + j < t1)
				hist[(size_t)(t + j) * ndig + d] = run;
			run += v[j];
		}
	}
}

/* ---- launch 3: rank and scatter ------------------------------------------- */
template <class Source, bool WORDS, bool LAST>
__global__ __launch_bounds__(WG) void dlv_scatter(Source s, uint32_t shift, uint32_t nbits,
						  const uint32_t *hist, uint32_t *dtotal,
						  uint32_t *dst)
{
	__shared__ __attribute__((aligned(16))) uint32_t s_a[T];
	__shared__ uint32_t s_dst[T];
	__shared__ uint32_t s_key[LAST ? 1u : T];
	__shared__ uint16_t s_cnt[WAVES][RADIX];
	__shared__ uint32_t s_tb[RADIX];
	__shared__ uint32_t s_gb[RADIX];
	__shared__ uint32_t s_ws[WAVES];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint32_t ndig = 1u << nbits, base = blockIdx.x * T;
	const uint32_t first = base + wave * WAVE_PKTS + lane;   /* run r: first + 64 r */
	const uint64_t below = (1ull << lane) - 1ull;
	uint32_t key[IPL], idx[IPL], rank[IPL];
	uint32_t valid = 0;

	/* the digit totals served launch 2 of this pass: cleared for the next */
	if (blockIdx.x == 0)
		for (uint32_t d = tid; d < RADIX; d += WG)
			dtotal[d] = 0;
	for (uint32_t d = lane; d < ndig; d += 64u)
		s_cnt[wave][d] = 0;
	for (uint32_t d = tid; d < ndig; d += WG)
		s_gb[d] = hist[(size_t)blockIdx.x * ndig + d];

	if (WORDS && s.num - base >= T && ((uintptr_t)s.src & 15u) == 0) {
		const uint4 *p = (const uint4 *)(s.src + base);

#pragma unroll
		for (uint32_t k = 0; k < IPL / 4u; k++)
			((uint4 *)s_a)[k * WG + tid] = p[k * WG + tid];
		__syncthreads();
#pragma unroll
		for (uint32_t r = 0; r < IPL; r++) {
			idx[r] = first + 64u * r;
			key[r] = s.key(s_a[idx[r] - base]);
		}
		valid = (1u << IPL) - 1u;
	} else {
#pragma unroll
		for (uint32_t r = 0; r < IPL; r++) {
			const uint32_t i = first + 64u * r;

			key[r] = 0;
			idx[r] = i;
			if (i < s.num) {
				if (WORDS) {
					key[r] = s.key(s.src[i]);
				} else {
					const uint2 p = ((const uint2 *)s.src)[i];

					key[r] = p.x;
					idx[r] = p.y;
				}
				valid |= 1u << r;
			}
		}
	}
	__syncthreads();

	/* rank within the wave, run by run in arrival order */
#pragma unroll
	for (uint32_t r = 0; r < IPL; r++) {
		const bool ok = (valid >> r) & 1u;
		const uint32_t d = (key[r] >> shift) & (ndig - 1u);
		const uint64_t peers = match_lanes(d, nbits, __ballot(ok));
		const uint32_t seen = s_cnt[wave][d];

		rank[r] = seen + (uint32_t)__popcll(peers & below);
		/* every lane of the wave has read its counter before the lowest
		 * peer advances it, and the next run reads it after that */
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
		if (ok && !(peers & below))
			s_cnt[wave][d] = (uint16_t)(seen + (uint32_t)__popcll(peers));
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
	}
	__syncthreads();

	/* per digit over the waves: s_cnt -> packets of the digit in the waves
	 * before; s_tb <- the tile's total */
	for (uint32_t d = tid; d < ndig; d += WG) {
		uint32_t run = 0;

#pragma unroll
		for (uint32_t w = 0; w < WAVES; w++) {
			const uint32_t c = s_cnt[w][d];

			s_cnt[w][d] = (uint16_t)run;
			run += c;
		}
		s_tb[d] = run;
	}
	__syncthreads();

	/* over the digits: s_tb -> first slot of the digit in the staged tile;
	 * s_gb -> what turns a staged slot into the global position */
	{
		constexpr uint32_t DPL = RADIX / WG;
		uint32_t v[DPL], sum = 0;

#pragma unroll
		for (uint32_t j = 0; j < DPL; j++) {
			const uint32_t d = tid * DPL + j;

			v[j] = d < ndig ? s_tb[d] : 0u;
			sum += v[j];
		}
		uint32_t run = block_excl_scan(sum, s_ws);

#pragma unroll
		for (uint32_t j = 0; j < DPL; j++) {
			const uint32_t d = tid * DPL + j;

			if (d < ndig) {
				s_tb[d] = run;
				s_gb[d] -= run;
			}
			run += v[j];
		}
	}
	__syncthreads();

#pragma unroll
	for (uint32_t r = 0; r < IPL; r++) {
		if ((valid >> r) & 1u) {
			const uint32_t d = (key[r] >> shift) & (ndig - 1u);
			const uint32_t slot = s_tb[d] + s_cnt[wave][d] + rank[r];

			s_a[slot] = idx[r];
			s_dst[slot] = slot + s_gb[d];
			if (!LAST)
				s_key[slot] = key[r];
		}
	}
	__syncthreads();

	const uint32_t cnt = min(T, s.num - base);

	for (uint32_t i = tid; i < cnt; i += WG) {
		const uint32_t g = s_dst[i];

		if (g >= s.num)     /* cannot happen with launch 2's bases */
			continue;
		if (LAST)
			dst[g] = s_a[i];
		else
			((uint2 *)dst)[g] = make_uint2(s_key[i], s_a[i]);
	}
}

__global__ void dlv_clear(uint32_t *p, uint32_t words)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;

	if (i < words)
		p[i] = 0;
}


inline int clear(uint32_t *p, uint32_t words, hipStream_t s)
{
	if (words)
		hipLaunchKernelGGL(dlv_clear, dim3((words + 255u) / 256u), dim3(256), 0, s, p, words);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

/* what a partition writes and works in */
struct Ws {
	uint32_t *order;    /* num packet indices, by key */
	uint32_t *offsets;  /* nbuckets + 1 */
	uint32_t  nbuckets; /* B: every key is < B */
	uint32_t  key_bits; /* dlv_key_bits(B) */
	uint32_t *hist;     /* [tiles << dlv_bits0(key_bits)]: counts, then global bases */
	uint32_t *dtotal;   /* [DLV_RADIX] digit totals of the running pass (zero
			     * between passes) */
	uint32_t *bcount;   /* [B] key counts, two-pass plans only (zero between calls) */
	uint32_t *pairs;    /* num x {key, index}, two-pass plans only */
};

/* the launches of one partition of src.num > 0 packets, on stream s */
template <class Source>
int partition(Source src, const Ws &a, hipStream_t s)
{
	const uint32_t ntiles = (src.num + T - 1u) / T;
	const uint32_t bits0 = dlv_bits0(a.key_bits), bits1 = a.key_bits - bits0;
	const uint32_t groups0 = ((1u << bits0) + 63u) / 64u;
	const bool two = bits1 != 0;

	hipLaunchKernelGGL((dlv_hist<Source, true>), dim3(ntiles), dim3(WG), 0, s, src, 0u, bits0,
			   a.key_bits, a.hist, a.dtotal, two ? a.bcount : nullptr);
	hipLaunchKernelGGL(dlv_scan, dim3(groups0), dim3(SCAN_WG), 0, s, a.hist, a.dtotal, ntiles,
			   bits0, two ? nullptr : a.offsets, a.nbuckets, src.num,
			   (uint32_t *)nullptr, groups0);
	if (!two) {
		hipLaunchKernelGGL((dlv_scatter<Source, true, true>), dim3(ntiles), dim3(WG), 0, s,
				   src, 0u, bits0, a.hist, a.dtotal, a.order);
		return hipGetLastError() == hipSuccess ? 0 : -EIO;
	}
	const uint32_t groups1 = ((1u << bits1) + 63u) / 64u;

	hipLaunchKernelGGL((dlv_scatter<Source, true, false>), dim3(ntiles), dim3(WG), 0, s, src, 0u,
			   bits0, a.hist, a.dtotal, a.pairs);
	src.src = a.pairs;
	hipLaunchKernelGGL((dlv_hist<Source, false>), dim3(ntiles), dim3(WG), 0, s, src, bits0, bits1,
			   bits1, a.hist, a.dtotal, (uint32_t *)nullptr);
	hipLaunchKernelGGL(dlv_scan, dim3(groups1 + 1u), dim3(SCAN_WG), 0, s, a.hist, a.dtotal,
			   ntiles, bits1, a.offsets, a.nbuckets, src.num, a.bcount, groups1);
	hipLaunchKernelGGL((dlv_scatter<Source, false, true>), dim3(ntiles), dim3(WG), 0, s, src,
			   bits0, bits1, a.hist, a.dtotal, a.order);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

} /* namespace rp */
} /* namespace */

#endif /* ODPG_RADIX_PASS_H_ */
