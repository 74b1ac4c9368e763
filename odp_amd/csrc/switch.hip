/* SPDX-License-Identifier: BSD-3-Clause
 *
 * L2 learning-switch forwarding of a device-resident batch
 * (include/odpg_switch.h): the sequential loop of the reference's
 * forward_packets, resolved in parallel.
 *
 * The one dependency between packets is rule 6: packet i's lookup of its
 * destination slot sees the last write to that slot by a packet j <= i, or the
 * table as it stood before the call. Every learning packet writes exactly its
 * source slot, so "the last writer of slot s up to i" is a predecessor query
 * on the ascending list of s's writers. Those lists are what a stable
 * partition of the packet indices by source slot yields: slot s's writers are
 * order[offsets[s] .. offsets[s + 1]), ascending because the partition is
 * stable. The partition is radix_pass.h's, the one deliver.hip runs on verdict
 * words, on a 17-bit key: the source slot, or 65536 for a dropped packet (a
 * bucket nobody looks up), as two digits of 9 and 8 bits. No atomic decides an
 * order, so the lists and everything derived from them are the same on every
 * run. The predecessor is found by binary search, at most 24 steps whatever
 * the MACs are: a batch whose sources all share one slot costs n log n.
 *
 * Ten launches, ordered by the stream alone; no kernel waits for another lane,
 * wave or workgroup, and every loop is bounded by the batch or table size.
 *   sw_key      a lane per packet. The twelve address bytes in one aligned
 *               16-byte load (n >= 14, so inside align16(n)), rules 1-3, the
 *               CRC32C of both addresses, a 16-byte record and the partition
 *               key. CRC32C with initial value 0 is linear in the message: the
 *               CRC of six bytes is the XOR of six lookups, one per byte
 *               position, in six 1 KiB tables the workgroup fills in LDS (lane
 *               b runs byte b through 8, 16, .. 48 shift steps). The lookups
 *               are independent; the one-table form chains six.
 *   dlv_*       the partition: five launches (radix_pass.h).
 *   sw_resolve  a lane per packet, a workgroup per tile of 256. Upper bound of
 *               i in the run of its destination slot; the predecessor's source
 *               bytes come from its record, written before this launch and
 *               immutable during it. No predecessor: the old table entry with
 *               the aging test. Stores out[i] and the packet's port mask, then
 *               counts the tile per port (one ballot per port, wave counts
 *               summed through LDS) and per kind.
 *   sw_commit   a lane per slot: a non-empty run's last writer's entry. A
 *               launch of its own after sw_resolve, so every read of the old
 *               table precedes every write.
 *   sw_scan     a workgroup per column (a port, or one of the four totals), a
 *               contiguous range of the tiles per lane: the running sum over
 *               the tiles in place (a tile's count becomes its first position
 *               in the port's list), port_offsets and the totals.
 *   sw_lists    a workgroup per tile: a lane's position in port p's list is
 *               the tile's base, plus the waves before it, plus the peers
 *               below it in the ballot. Ascending by construction.
 *
 * LDS, bytes: sw_key 6144 (the tables); sw_resolve 4 x 35 x 4 = 560;
 * sw_scan 64; sw_lists 4 x 32 x 4 = 512. Registers:
 * DESIGN "L2 switch".
 */
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>

#include "switch.h"
#include "radix_pass.h"

namespace {

constexpr uint32_t T = SW_TILE;
constexpr uint32_t WG = 256;
constexpr uint32_t WAVES = WG / 64;
constexpr uint32_t SCAN_WG = 1024;
constexpr uint32_t POLY = 0x82F63B78u;      /* CRC32C, reflected */
constexpr uint32_t K_NONE = 0xFFu;          /* a lane beyond the batch */

static_assert(T == WG, "a tile is one workgroup, a lane per packet");
static_assert(sizeof(odpg_switch_rec) == 16, "layout");
static_assert(SW_COLS <= 64, "a column per lane of a wave");
static_assert(SW_BUCKETS <= (1u << SW_KEY_BITS) && SW_KEY_BITS <= 2u * DLV_DIGIT_BITS, "key");

typedef odpg_switch_args Args;

/* partition source: the key words sw_key wrote */
struct Keys {
	const uint32_t *src;
	uint32_t num;

	__device__ __forceinline__ uint32_t key(uint32_t w) const
	{
		return min(w, SW_SLOTS);
	}
};

__device__ __forceinline__ uint64_t dst_of(const uint4 r)
{
	return (uint64_t)r.x | (uint64_t)(r.y & 0xFFFFu) << 32;
}

__device__ __forceinline__ uint64_t src_of(const uint4 r)
{
	return (uint64_t)(r.y >> 16) | (uint64_t)r.z << 16;
}

/* mac_tbl_entry_t on little-endian (odp_switch.c:53-61) */
__device__ __forceinline__ uint64_t entry_of(const uint4 r, uint32_t tick)
{
	return src_of(r) | (uint64_t)(r.w & 0xFFu) << 48 | (uint64_t)tick << 56;
}

/* CRC32C (initial value 0) of the six bytes of m through the per-position tables */
__device__ __forceinline__ uint32_t crc6(const uint32_t (*tab)[256], uint64_t m)
{
	const uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);

	return tab[0][lo & 0xFFu] ^ tab[1][(lo >> 8) & 0xFFu] ^ tab[2][(lo >> 16) & 0xFFu] ^
	       tab[3][lo >> 24] ^ tab[4][hi & 0xFFu] ^ tab[5][(hi >> 8) & 0xFFu];
}

/* ---- launch 1: rules 1-3, slots, records, partition keys ------------------- */
__global__ __launch_bounds__(WG) void sw_key(Args a)
{
	__shared__ uint32_t s_crc[6][256];
	const uint32_t tid = threadIdx.x, i = blockIdx.x * WG + tid;

	/* byte `tid` at position k of six: 8 steps for itself, 8 per zero byte after it */
	{
		uint32_t x = tid;

#pragma unroll
		for (int k = 5; k >= 0; k--) {
#pragma unroll
			for (uint32_t b = 0; b < 8u; b++)
				x = (x >> 1) ^ ((x & 1u) ? POLY : 0u);
			s_crc[k][tid] = x;
		}
	}
	__syncthreads();
	if (i >= a.src.num)
		return;
	uint32_t off = 0, len = a.src.stride;

	if (a.src.desc) {
		const uint2 d = ((const uint2 *)a.src.desc)[i];

		off = d.x;
		len = d.y;
	}
	const uint32_t port = a.src.port_in ? a.src.port_in[i] : a.src.uniform_port;
	uint4 v = make_uint4(0u, 0u, 0u, 0u);
	uint32_t kind = SW_K_FWD, sslot = SW_SLOTS, dslot = 0;

	if (len < 14u) {
		kind = ODPG_SWITCH_DROP_FRAME;
	} else {
		/* 14 <= len: the first unit is inside align16(len) */
		v = *(const uint4 *)(a.src.frames +
				     (a.src.desc ? (uint64_t)off : (uint64_t)i * a.src.stride));
		const uint64_t d = dst_of(v), s = src_of(v);

		if (port >= a.num_ports) {
			kind = ODPG_SWITCH_DROP_PORT;
		} else if (s == 0xFFFFFFFFFFFFull || s == 0 || d == 0) {
			kind = ODPG_SWITCH_DROP_FRAME;
		} else {
			sslot = crc6(s_crc, s) & (SW_SLOTS - 1u);
			dslot = crc6(s_crc, d) & (SW_SLOTS - 1u);
		}
	}
	((uint4 *)a.rec)[i] = make_uint4(v.x, v.y, v.z, (port & 0xFFu) | kind << 8 | dslot << 16);
	a.skey[i] = sslot;
}

/* ---- launch 7: rules 6-8, port masks, tile counts --------------------------- */
__global__ __launch_bounds__(WG) void sw_resolve(Args a)
{
	__shared__ uint32_t s_cnt[WAVES][SW_COL_ENTRIES];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint32_t i = blockIdx.x * T + tid, num = a.src.num, P = a.num_ports;
	const uint32_t all = P >= 32u ? 0xFFFFFFFFu : (1u << P) - 1u;
	uint32_t kind = K_NONE, mask = 0;

	if (i < num) {
		const uint4 r = ((const uint4 *)a.rec)[i];
		const uint32_t port = r.w & 0xFFu, dslot = r.w >> 16;
		const uint64_t d = dst_of(r);
		uint32_t outp = 0;

		kind = (r.w >> 8) & 0xFFu;
		if (kind == SW_K_FWD) {
			kind = ODPG_SWITCH_FLOOD;
			if (d != 0xFFFFFFFFFFFFull) {
				const uint32_t lo = a.offsets[dslot];
				uint32_t l = lo, h = min(a.offsets[dslot + 1u], num);
				uint64_t e;
				bool live = true;

				/* first writer of the slot beyond i; h - l < 2^25 */
				for (uint32_t step = 0; step < 26u && l < h; step++) {
					const uint32_t m = (l + h) >> 1;

					if (a.order[m] <= i)
						l = m + 1u;
					else
						h = m;
				}
				if (l > lo) {
					const uint32_t j = a.order[l - 1u];

					/* a writer of this call: tick distance 0 */
					e = entry_of(j < num ? ((const uint4 *)a.rec)[j] : r, a.cur_tick);
				} else {
					e = a.table[dslot];
					const uint32_t t1 = (uint32_t)(e >> 56), t2 = a.cur_tick;
					const uint32_t diff = t1 < t2 ? t2 - t1
							    : t1 > t2 ? (255u + t2 - t1) & 0xFFu : 0u;

					live = diff <= ODPG_SWITCH_AGING_TIME;
				}
				if ((e & 0xFFFFFFFFFFFFull) == d && live) {
					kind = ODPG_SWITCH_UNICAST;
					outp = (uint32_t)(e >> 48) & 0xFFu;
				}
			}
			mask = kind == ODPG_SWITCH_UNICAST ? (outp < 32u ? 1u << outp : 0u) & all
							   : all & ~(1u << port);
		}
		a.dst.out[i] = kind << 8 | outp;
		a.mask[i] = mask;
	}

	/* lane c keeps column c's count of its wave */
	uint32_t mine = 0;

	for (uint32_t p = 0; p < P; p++) {
		const uint32_t c = (uint32_t)__popcll(__ballot((mask >> p) & 1u));

		if (lane == p)
			mine = c;
	}
	{
		const uint32_t u = (uint32_t)__popcll(__ballot(kind == ODPG_SWITCH_UNICAST));
		const uint32_t f = (uint32_t)__popcll(__ballot(kind == ODPG_SWITCH_FLOOD));
		const uint32_t d = (uint32_t)__popcll(__ballot(kind == ODPG_SWITCH_DROP_FRAME ||
							       kind == ODPG_SWITCH_DROP_PORT));

		if (lane >= SW_COL_KIND)
			mine = lane == SW_COL_KIND ? u : lane == SW_COL_KIND + 1u ? f : d;
	}
	if (lane < SW_COL_ENTRIES)
		s_cnt[wave][lane] = mine;
	__syncthreads();
	if (tid < SW_COLS) {
		uint32_t c = 0;

		if (tid == SW_COL_ENTRIES) {
			for (uint32_t p = 0; p < P; p++)
				for (uint32_t w = 0; w < WAVES; w++)
					c += s_cnt[w][p];
		} else {
#pragma unroll
			for (uint32_t w = 0; w < WAVES; w++)
				c += s_cnt[w][tid];
		}
		a.tcnt[(size_t)tid * gridDim.x + blockIdx.x] = c;
	}
}

/* ---- launch 8: rule 9 -------------------------------------------------------- */
__global__ __launch_bounds__(WG) void sw_commit(Args a)
{
	const uint32_t s = blockIdx.x * WG + threadIdx.x;

	if (s >= SW_SLOTS)
		return;
	const uint32_t lo = a.offsets[s], hi = min(a.offsets[s + 1u], a.src.num);

	if (hi > lo) {
		const uint32_t j = a.order[hi - 1u];

		if (j < a.src.num)
			a.table[s] = entry_of(((const uint4 *)a.rec)[j], a.cur_tick);
	}
}

/* ---- launch 9: list bases of every tile, port_offsets, totals ----------------
 * Workgroup c: column c over the tiles, a contiguous range of them per lane. */
__global__ __launch_bounds__(SCAN_WG) void sw_scan(Args a, uint32_t ntiles)
{
	__shared__ uint32_t s_ws[SCAN_WG / 64u];
	const uint32_t tid = threadIdx.x, c = blockIdx.x;

	if (c >= a.num_ports && c < SW_COL_KIND)
		return;
	uint32_t *col = a.tcnt + (size_t)c * ntiles;
	const uint32_t per = (ntiles + SCAN_WG - 1u) / SCAN_WG;
	const uint32_t t0 = min(ntiles, tid * per), t1 = min(ntiles, t0 + per);
	uint32_t sum = 0;

	for (uint32_t t = t0; t < t1; t++)
		sum += col[t];
	uint32_t run = rp::block_excl_scan(sum, s_ws);

	if (tid == SCAN_WG - 1u) {
		if (c < SW_COL_KIND) {
			a.dst.port_offsets[2u * c] = 0;
			a.dst.port_offsets[2u * c + 1u] = run + sum;
		} else {
			((uint32_t *)a.dst.total)[c - SW_COL_KIND] = run + sum;
		}
	}
	if (c < SW_COL_KIND) {
		for (uint32_t t = t0; t < t1; t++) {
			const uint32_t v = col[t];

			col[t] = run;
			run += v;
		}
	}
}

/* ---- launch 10: the per-port lists ------------------------------------------- */
__global__ __launch_bounds__(WG) void sw_lists(Args a)
{
	__shared__ uint32_t s_cnt[WAVES][ODPG_SWITCH_MAX_PORTS];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint32_t i = blockIdx.x * T + tid, P = a.num_ports;
	const uint64_t below = (1ull << lane) - 1ull;
	const uint32_t mask = i < a.src.num ? a.mask[i] : 0u;
	uint32_t mine = 0;

	for (uint32_t p = 0; p < P; p++) {
		const uint32_t c = (uint32_t)__popcll(__ballot((mask >> p) & 1u));

		if (lane == p)
			mine = c;
	}
	if (lane < ODPG_SWITCH_MAX_PORTS)
		s_cnt[wave][lane] = mine;
	__syncthreads();
	for (uint32_t p = 0; p < P; p++) {
		const bool in = (mask >> p) & 1u;
		const uint64_t peers = __ballot(in);
		uint32_t pos = a.tcnt[(size_t)p * gridDim.x + blockIdx.x] +
			       (uint32_t)__popcll(peers & below);

		for (uint32_t w = 0; w < wave; w++)
			pos += s_cnt[w][p];
		if (in && pos < a.dst.list_stride)
			a.dst.lists[(size_t)p * a.dst.list_stride + pos] = i;
	}
}

} /* namespace */

extern "C" int odpg_launch_switch_clear(uint32_t *p, uint32_t words, hipStream_t s)
{
	return rp::clear(p, words, s);
}

extern "C" int odpg_launch_switch(const odpg_switch_args *a, hipStream_t s)
{
	const uint32_t num = a->src.num, ntiles = (num + T - 1u) / T;

	if (num) {
		const Keys keys = {a->skey, num};
		const rp::Ws ws = {a->order, a->offsets, SW_BUCKETS, SW_KEY_BITS,
				   a->hist, a->dtotal, a->bcount, a->pairs};

		hipLaunchKernelGGL(sw_key, dim3(ntiles), dim3(WG), 0, s, *a);
		if (rp::partition(keys, ws, s))
			return -EIO;
		hipLaunchKernelGGL(sw_resolve, dim3(ntiles), dim3(WG), 0, s, *a);
		hipLaunchKernelGGL(sw_commit, dim3(SW_SLOTS / WG), dim3(WG), 0, s, *a);
	}
	hipLaunchKernelGGL(sw_scan, dim3(SW_COLS), dim3(SCAN_WG), 0, s, *a, ntiles);
	if (num)
		hipLaunchKernelGGL(sw_lists, dim3(ntiles), dim3(WG), 0, s, *a);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
