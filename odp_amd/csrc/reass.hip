/* SPDX-License-Identifier: BSD-3-Clause
 *
 * IPv4 reassembly of a device-resident batch (include/odpg_reass.h): the
 * many-to-one counterpart of lso.hip. Fragments are grouped by flow with no
 * sort: a fragment's place in its datagram, L0 + hl0 + 8 off, is known from
 * its own header, so all a group needs is the test whether its members tile
 * [0, W). That test is five integer conditions on the group (exactly one
 * member with MF == 0; a member at offset 0; every MF member has some member
 * starting at its end; sum of payloads == W; hl0 + W <= 65535): the successor
 * chain from offset 0 strictly increases and can only stop at the one
 * terminal, so it covers [0, W), and with p > 0 any member off the chain makes
 * the sum exceed W.
 *
 * Seven launches, ordered by the stream alone; no kernel waits for another
 * lane, wave or workgroup, and every probe loop is bounded by the table size.
 *   reass_clear  flow table, position table and group records of this call
 *                (tables of tsize = pow2 >= 2 num slots, so they cannot fill).
 *   reass_key    a lane per packet, a wave per tile of 64: the header through
 *                aligned 16-byte loads and the funnel, rules 1-3, a 16-byte
 *                record per packet. A fragment claims or finds its flow's slot
 *                (atomicCAS EMPTY -> i; on a taken slot the 11 key bytes are
 *                compared with the owner's, read from the owner's immutable
 *                source frame), the owner being the group's leader; inserts
 *                (leader, 8 off) as one 64-bit key into the position table;
 *                and adds into the leader's group record with integer
 *                atomics. A wave without fragments leaves on one ballot.
 *   reass_link   every MF fragment looks (leader, 8 off + p) up; a miss sets
 *                the group's flag. A launch of its own: all inserts are in.
 *   reass_emit   a lane per packet: status[i]; lane i emits if WHOLE, or if i
 *                is the largest index of a complete group; output length per
 *                packet, sums of outputs, units, held and bad per tile.
 *   reass_scan   one workgroup: exclusive scan of the tile sums, total,
 *                held_offsets.
 *   reass_place  in-tile prefix: desc[j], origin[j], the output's base unit
 *                (per WHOLE packet, or in the group record), held[]; the one
 *                lane whose output is the first that does not fit stores
 *                total.copied (no atomics: one per tile into one word cost
 *                more than the copy on an IMIX batch).
 *   reass_copy   a workgroup of 256 lanes per tile of 64 source packets; where
 *                the bytes move.
 *
 * reass_copy is source-centric. Every source packet that is copied is one run
 * of bytes: a WHOLE frame [0, len) to its output; member 0 of a group
 * [0, L0 + tl0) (header and payload are contiguous in both) to the output's
 * start; any other member its payload to byte L0 + hl0 + 8 off of the output.
 * The destination units a run touches are numbered across the tile (a scan in
 * LDS); lane l of step k owns unit 256 k + l and searches from unit to packet
 * only when its unit leaves the packet it holds. A unit wholly inside the run
 * is built from the two aligned source units around it by the funnel of
 * unit_copy.h and stored as 16 bytes. The up to 15 bytes at each end of a run
 * share their unit with the neighbouring fragment (another lane, maybe another
 * workgroup): they are written with byte, short and dword stores as alignment
 * allows, never by a read-modify-write of the unit. The terminal member (and a
 * WHOLE frame) also writes the zero padding up to align16. The one or two
 * units of member 0 that hold tot_len, the fragment field and the checksum
 * are skipped by the bulk and written by one lane per group, which sums the
 * header and patches the bytes in registers. All reads stay inside
 * [offset, offset + align16(len)): a run ends at L + tl <= len.
 *
 * LDS, bytes: reass_copy 1552 (five words per packet, the unit scan);
 * reass_scan 64. Registers: DESIGN "Reassembly".
 */
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>
#include <algorithm>

#include "reass.h"
#include "unit_copy.h"

namespace {

constexpr uint32_t T = REASS_TILE;
constexpr uint32_t WG = 256;
constexpr uint32_t DEPTH = 4;               /* units a lane keeps in flight (two loads each) */
constexpr uint32_t SCAN_WG = 512;            /* 1024 lanes: 128 VGPRs and spills */
constexpr uint32_t NONE = REASS_NONE;
constexpr unsigned long long EMPTY64 = ~0ull;
constexpr uint32_t M_PAD = 16u, M_PATCH = 32u;   /* s_misc: dl | flags | L0 << 16 */

static_assert(T == 64, "a tile is one wave");
static_assert(sizeof(odpg_reass_pk) == 16 && sizeof(odpg_reass_grp) == 32, "layout");

typedef odpg_reass_args Args;

__device__ __forceinline__ uint32_t be16_hi(uint32_t w)   /* bytes 2, 3 of a loaded dword */
{
	return ((w >> 8) & 0xFF00u) | (w >> 24);
}

__device__ __forceinline__ uint32_t mix(uint32_t h)
{
	h ^= h >> 16;
	h *= 0x85EBCA6Bu;
	h ^= h >> 13;
	h *= 0xC2B2AE35u;
	return h ^ (h >> 16);
}

__device__ __forceinline__ const uint8_t *frame_at(const Args &a, uint32_t off, uint32_t i)
{
	return a.src.frames + (a.src.desc ? (uint64_t)off : (uint64_t)i * a.src.stride);
}

/* packet i's descriptor and L3 offset; true if [L, L + 20) lies in the frame,
 * then h = bytes [L, L + 16) and h4 = bytes [L + 16, L + 20) */
__device__ __forceinline__ bool load_hdr(const Args &a, uint32_t i, uint32_t &off, uint32_t &len,
					 uint32_t &L, uint4 &h, uint32_t &h4)
{
	off = 0;
	len = a.src.stride;
	if (a.src.desc) {
		const uint2 d = ((const uint2 *)a.src.desc)[i];

		off = d.x;
		len = d.y;
	}
	L = a.src.l3_offset
		? *(const uint16_t *)((const uint8_t *)a.src.l3_offset + (uint64_t)i * a.src.l3_stride)
		: a.src.uniform_l3;
	if (L == ODPG_OFFSET_INVALID || L + 20u > len)
		return false;
	/* L + 20 <= len: the units that hold [L, L + 20) are inside align16(len) */
	const uint4 *u = (const uint4 *)(frame_at(a, off, i) + (L & ~15u));
	const uint32_t sh = L & 15u;
	const uint4 u0 = u[0], u1 = u[1];
	const uint4 u2 = sh > 12u ? u[2] : make_uint4(0u, 0u, 0u, 0u);

	h = funnel(u0, u1, sh);
	h4 = funnel(u1, u2, sh).x;
	return true;
}

struct Pkt {
	uint32_t off, len, L, p, hl, fo, mf, kind;
};

__device__ __forceinline__ Pkt decode(const uint4 r)
{
	Pkt p;

	p.off = r.x;
	p.len = r.y;
	p.L = r.z & 0xFFFFu;
	p.p = r.z >> 16;
	p.hl = r.w & 0xFFu;
	p.fo = (r.w >> 8) & 0x1FFFu;
	p.mf = (r.w >> 21) & 1u;
	p.kind = r.w >> 24;
	return p;
}

/* ---- launch 0: tables and group records of this call ----------------------- */
__global__ __launch_bounds__(WG) void reass_clear(Args a)
{
	const uint32_t step = gridDim.x * WG, t0 = blockIdx.x * WG + threadIdx.x;

	for (uint32_t s = t0; s < a.tsize; s += step) {
		a.flow[s] = NONE;
		a.pos[s] = EMPTY64;
	}
	for (uint32_t i = t0; i < a.src.num; i += step) {
		uint4 *g = (uint4 *)&a.grp[i];

		g[0] = make_uint4(0u, 0u, 0u, 0u);           /* sum_p, nterm, W */
		g[1] = make_uint4(NONE, 0u, 0u, NONE);       /* first, last, miss, base */
	}
}

/* ---- launch 1: rules 1-3, flow and position tables, group sums ------------- */
__global__ __launch_bounds__(WG) void reass_key(Args a)
{
	const uint32_t i = blockIdx.x * WG + threadIdx.x, num = a.src.num, mask = a.tsize - 1u;
	uint32_t kind = REASS_K_WHOLE, p = 0, fo = 0, mf = 0, k0 = 0, k1 = 0, k2 = 0;

	if (i < num) {
		uint32_t off, len, L, h4, hl = 0;
		uint4 h;

		if (load_hdr(a, i, off, len, L, h, h4)) {
			const uint32_t ihl = h.x & 15u, f = be16_hi(h.y);

			if (((h.x >> 4) & 15u) == 4u && ihl >= 5u && L + 4u * ihl <= len &&
			    (f & 0x3FFFu)) {
				const uint32_t tl = be16_hi(h.x);

				hl = 4u * ihl;
				mf = (f >> 13) & 1u;
				fo = f & 0x1FFFu;
				p = tl - hl;
				kind = (tl <= hl || L + tl > len || (mf && (p & 7u))) ? REASS_K_BAD
										       : REASS_K_FRAG;
				k0 = h.w;
				k1 = h4;
				k2 = (h.y & 0xFFFFu) | (h.z & 0xFF00u) << 8;
			}
		}
		if (kind != REASS_K_FRAG)
			p = fo = mf = 0;
		((uint4 *)a.pk)[i] = make_uint4(off, len, (L & 0xFFFFu) | p << 16,
						hl | fo << 8 | mf << 21 | kind << 24);
	}
	if (!__ballot(kind == REASS_K_FRAG))
		return;
	if (kind != REASS_K_FRAG)
		return;
	uint32_t leader = NONE, s = mix(k0 ^ mix(k1 ^ mix(k2))) & mask;

	for (uint32_t n = 0; n < a.tsize; n++, s = (s + 1u) & mask) {
		const uint32_t own = atomicCAS(&a.flow[s], NONE, i);

		if (own == NONE) {
			leader = i;
			break;
		}
		/* the owner is a fragment: its header is in its frame, which nobody writes */
		uint32_t o_off, o_len, o_L, o4;
		uint4 o;

		load_hdr(a, own, o_off, o_len, o_L, o, o4);
		if (o.w == k0 && o4 == k1 && ((o.y & 0xFFFFu) | (o.z & 0xFF00u) << 8) == k2) {
			leader = own;
			break;
		}
	}
	a.lead[i] = leader;
	if (leader == NONE) {           /* not reached: the table has >= 2 num slots */
		a.pk[i].hofk = REASS_K_BAD << 24;
		return;
	}
	const uint32_t start = 8u * fo;
	const unsigned long long key = (unsigned long long)leader << 32 | start;

	s = mix(leader ^ mix(start)) & mask;
	for (uint32_t n = 0; n < a.tsize; n++, s = (s + 1u) & mask) {
		const unsigned long long was = atomicCAS(&a.pos[s], EMPTY64, key);

		if (was == EMPTY64 || was == key)
			break;
	}
	odpg_reass_grp *g = &a.grp[leader];

	atomicAdd(&g->sum_p, (unsigned long long)p);
	if (!mf) {
		atomicAdd(&g->nterm, 1u);
		atomicMax(&g->W, start + p);
	}
	if (!fo)
		atomicMin(&g->first, i);
	atomicMax(&g->last, i);
}

/* ---- launch 2: does every MF member have a successor ----------------------- */
__global__ __launch_bounds__(WG) void reass_link(Args a)
{
	const uint32_t i = blockIdx.x * WG + threadIdx.x, mask = a.tsize - 1u;

	if (i >= a.src.num)
		return;
	const Pkt k = decode(((const uint4 *)a.pk)[i]);

	if (k.kind != REASS_K_FRAG || !k.mf)
		return;
	const uint32_t leader = a.lead[i], end = 8u * k.fo + k.p;
	const unsigned long long key = (unsigned long long)leader << 32 | end;
	uint32_t s = mix(leader ^ mix(end)) & mask;
	bool found = false;

	for (uint32_t n = 0; n < a.tsize; n++, s = (s + 1u) & mask) {
		const unsigned long long v = a.pos[s];

		found = v == key;
		if (found || v == EMPTY64)
			break;
	}
	if (!found)
		atomicOr(&a.grp[leader].miss, 1u);
}

/* ---- launch 3: status, who emits what, tile sums --------------------------- */
__global__ __launch_bounds__(WG) void reass_emit(Args a)
{
	const uint32_t tid = threadIdx.x, i = blockIdx.x * WG + tid, num = a.src.num;
	uint32_t e = NONE, held = 0, bad = 0;

	if (i < num) {
		const Pkt k = decode(((const uint4 *)a.pk)[i]);
		uint32_t st = ODPG_REASS_WHOLE;

		if (k.kind == REASS_K_WHOLE) {
			e = k.len;
		} else if (k.kind == REASS_K_BAD) {
			st = ODPG_REASS_BAD;
			bad = 1;
		} else {
			const odpg_reass_grp g = a.grp[a.lead[i]];
			bool complete = g.nterm == 1u && g.first != NONE && !g.miss && g.sum_p == g.W;

			if (complete) {
				const Pkt k0 = g.first == i ? k : decode(((const uint4 *)a.pk)[g.first]);

				complete = k0.hl + g.W <= 65535u;
				if (complete && g.last == i)
					e = k0.L + k0.hl + g.W;
			}
			st = complete ? ODPG_REASS_JOINED : ODPG_REASS_HELD;
			held = !complete;
		}
		a.dst.status[i] = (uint8_t)st;
		a.obase[i] = e;
	}
	uint32_t outs = e != NONE;
	uint64_t units = e != NONE ? units_of(e) : 0u;

	for (uint32_t off = 32; off; off >>= 1) {
		outs += __shfl_xor(outs, off);
		units += __shfl_xor(units, off);
		held += __shfl_xor(held, off);
		bad += __shfl_xor(bad, off);
	}
	const uint32_t tile = i / T;            /* T == the wave size */

	if ((tid & 63u) == 0 && tile * T < num) {
		a.touts[tile] = outs;
		a.tunits[tile] = units;
		a.theld[tile] = held;
		a.tbad[tile] = bad;
	}
}

/* ---- launch 4: tile sums -> tile bases, total, held_offsets ---------------- */
__global__ __launch_bounds__(SCAN_WG) void reass_scan(Args a)
{
	__shared__ uint64_t s_ws[SCAN_WG / 64];
	const uint32_t tid = threadIdx.x, num = a.src.num;
	const uint32_t ntiles = num / T + (num % T != 0);
	/* a lane owns `per` consecutive tiles: sums them, one scan over the
	 * lanes, then walks them again with its base */
	const uint32_t per = (ntiles + SCAN_WG - 1u) / SCAN_WG;
	const uint32_t t0 = min(tid * per, ntiles), t1 = min(t0 + per, ntiles);
	uint64_t su = 0, so = 0, sh = 0, sb = 0, au, ao, ah, ab;

	/* no aliases, so the loads of several tiles are in flight together */
	uint64_t *__restrict__ tu = a.tunits;
	uint32_t *__restrict__ to = a.touts, *__restrict__ th = a.theld;
	const uint32_t *__restrict__ tb = a.tbad;

#pragma unroll 8
	for (uint32_t t = t0; t < t1; t++) {
		su += tu[t];
		so += to[t];
		sh += th[t];
		sb += tb[t];
	}
	uint64_t bu = block_excl_scan<SCAN_WG / 64>(su, s_ws, &au);
	uint64_t bo = block_excl_scan<SCAN_WG / 64>(so, s_ws, &ao);
	uint64_t bh = block_excl_scan<SCAN_WG / 64>(sh, s_ws, &ah);

	block_excl_scan<SCAN_WG / 64>(sb, s_ws, &ab);
#pragma unroll 8
	for (uint32_t t = t0; t < t1; t++) {
		const uint64_t u = tu[t];
		const uint32_t o = to[t], h = th[t];

		tu[t] = bu;
		to[t] = (uint32_t)bo;
		th[t] = (uint32_t)bh;
		bu += u;
		bo += o;
		bh += h;
	}
	if (tid == 0) {
		a.dst.total->num_out = (uint32_t)ao;
		a.dst.total->copied = (uint32_t)ao;   /* reass_place: the first output that does not fit */
		a.dst.total->num_held = (uint32_t)ah;
		a.dst.total->num_bad = (uint32_t)ab;
		a.dst.total->bytes = au << 4;
		a.dst.held_offsets[0] = 0;
		a.dst.held_offsets[1] = (uint32_t)ah;
	}
}

/* ---- launch 5: descriptors, origins, output bases, the held list ----------- */
__global__ __launch_bounds__(WG) void reass_place(Args a)
{
	const uint32_t tid = threadIdx.x, i = blockIdx.x * WG + tid, num = a.src.num;
	const uint32_t tile = i / T;
	const bool in = i < num;
	const uint32_t e = in ? a.obase[i] : NONE;
	const uint32_t held = in && a.dst.status[i] == ODPG_REASS_HELD;
	const uint32_t outs = e != NONE;
	const uint64_t units = outs ? units_of(e) : 0u;
	const uint32_t io = wave_incl_scan(outs), ih = wave_incl_scan(held);
	const uint64_t iu = wave_incl_scan(units);

	if (outs) {
		const uint32_t j = a.touts[tile] + io - outs;
		const uint64_t base = a.tunits[tile] + iu - units;
		const Pkt k = decode(((const uint4 *)a.pk)[i]);
		odpg_reass_grp *g = k.kind == REASS_K_FRAG ? &a.grp[a.lead[i]] : nullptr;

		/* a written frame ends at or below 2^32: base < 2^28 */
		const bool fits = j < a.dst.max_out && ((base + units) << 4) <= a.dst.capacity;

		/* both limits are monotone in j: the outputs that fit are a prefix, and
		 * the one lane whose output is the first beyond it says how long it is
		 * (output j - 1 ends where j starts). No atomics. */
		if (!fits && (j == 0 || (j - 1u < a.dst.max_out && (base << 4) <= a.dst.capacity)))
			a.dst.total->copied = j;
		if (j < a.dst.max_out) {
			((uint2 *)a.dst.desc)[j] = fits ? make_uint2((uint32_t)(base << 4), e)
							: make_uint2(0u, 0u);
			a.dst.origin[j] = g ? g->first : i;
		}
		if (g) {
			if (fits)
				g->base = (uint32_t)base;
			a.obase[i] = NONE;
		} else {
			a.obase[i] = fits ? (uint32_t)base : NONE;
		}
	}
	if (held)
		a.dst.held[a.theld[tile] + ih - held] = i;
}

/* ---- launch 6: the bytes ----------------------------------------------------- */

/* bytes [x, x + 4) of a frame, any x, from aligned dwords inside [x, x + 4) */
__device__ __forceinline__ uint32_t load32u(const uint8_t *fr, uint32_t x)
{
	const uint32_t *q = (const uint32_t *)(fr + (x & ~3u));
	const uint32_t lo = q[0], hi = (x & 3u) ? q[1] : 0u;

	return __builtin_amdgcn_alignbyte(hi, lo, x & 3u);
}

/* the two big-endian 16-bit words of a loaded dword, added */
__device__ __forceinline__ uint32_t be_words(uint32_t w)
{
	return ((w & 0xFFu) << 8 | ((w >> 8) & 0xFFu)) + (((w >> 8) & 0xFF00u) | w >> 24);
}

/* byte x (0..15) of v = b */
__device__ __forceinline__ void put_byte(uint4 &v, uint32_t x, uint32_t b)
{
	const uint32_t sh = 8u * (x & 3u), m = ~(0xFFu << sh), w = (b & 0xFFu) << sh, k = x >> 2;

	v.x = k == 0u ? (v.x & m) | w : v.x;
	v.y = k == 1u ? (v.y & m) | w : v.y;
	v.z = k == 2u ? (v.z & m) | w : v.z;
	v.w = k == 3u ? (v.w & m) | w : v.w;
}

/* the low cnt (< 16) bytes of v to q, whose offset in its 16-byte unit is pos:
 * byte, short and dword stores, nothing outside [q, q + cnt) */
__device__ __forceinline__ void store_bytes(uint8_t *q, uint4 v, uint32_t pos, uint32_t cnt)
{
	const uint4 z = make_uint4(0u, 0u, 0u, 0u);

	if ((pos & 1u) && cnt) {
		*q = (uint8_t)v.x;
		v = funnel(v, z, 1u);
		q++;
		pos++;
		cnt--;
	}
	if ((pos & 2u) && cnt >= 2u) {
		*(uint16_t *)q = (uint16_t)v.x;
		v = funnel(v, z, 2u);
		q += 2;
		cnt -= 2u;
	}
#pragma unroll
	for (uint32_t t = 0; t < 3u; t++) {
		if (cnt >= 4u) {
			*(uint32_t *)q = v.x;
			v = make_uint4(v.y, v.z, v.w, 0u);
			q += 4;
			cnt -= 4u;
		}
	}
	if (cnt >= 2u) {
		*(uint16_t *)q = (uint16_t)v.x;
		v.x >>= 16;
		q += 2;
		cnt -= 2u;
	}
	if (cnt)
		*q = (uint8_t)v.x;
}

__global__ __launch_bounds__(WG) void reass_copy(Args a)
{
	__shared__ uint32_t s_start[T + 1];   /* destination units of the tile's runs, scanned */
	__shared__ uint32_t s_off[T];         /* source descriptor offset */
	__shared__ uint32_t s_s0[T];          /* first source byte of the run */
	__shared__ uint32_t s_nb[T];          /* bytes of the run */
	__shared__ uint32_t s_du[T];          /* destination unit of the run's first byte */
	__shared__ uint32_t s_misc[T];        /* that byte's place in it | M_* | L0 << 16 */
	const uint32_t tid = threadIdx.x, i0 = blockIdx.x * T, num = a.src.num;
	uint4 *dst = (uint4 *)a.dst.frames;
	/* wave 0 keeps its packet's run for the patch at the end */
	uint32_t m_off = 0, m_du = 0, m_misc = 0, m_hl = 0, m_W = 0;

	if (tid < T) {
		const uint32_t i = i0 + tid;
		uint32_t s0 = 0, nb = 0, D = 0, base = NONE, misc = 0;

		if (i < num) {
			const Pkt k = decode(((const uint4 *)a.pk)[i]);

			m_off = k.off;
			if (k.kind == REASS_K_WHOLE) {
				base = a.obase[i];
				nb = k.len;
				misc = M_PAD;
			} else if (k.kind == REASS_K_FRAG) {
				const odpg_reass_grp g = a.grp[a.lead[i]];

				base = g.base;          /* set: the group is complete and fits */
				if (base != NONE && g.first == i) {
					nb = k.L + k.hl + k.p;
					misc = M_PATCH | k.L << 16;
					m_hl = k.hl;
					m_W = g.W;
				} else if (base != NONE) {
					const Pkt k0 = decode(((const uint4 *)a.pk)[g.first]);

					s0 = k.L + k.hl;
					nb = k.p;
					D = k0.L + k0.hl + 8u * k.fo;
					misc = k.mf ? 0u : M_PAD;
				}
			}
		}
		if (base == NONE)
			nb = 0;
		misc |= D & 15u;
		m_du = base + (D >> 4);
		m_misc = nb ? misc : 0u;
		const uint32_t nu = nb ? ((D & 15u) + nb + 15u) >> 4 : 0u;
		const uint32_t iu = wave_incl_scan(nu);     /* <= 64 * 8194 */

		s_off[tid] = m_off;
		s_s0[tid] = s0;
		s_nb[tid] = nb;
		s_du[tid] = m_du;
		s_misc[tid] = misc;
		s_start[tid] = iu - nu;
		if (tid == T - 1u)
			s_start[T] = iu;
	}
	__syncthreads();
	const uint32_t total = s_start[T];

	/* ---- bulk ---- */
	{
		uint32_t f = 0, lo = 0, hi = 0;     /* the lane's packet: units [lo, hi) */
		uint32_t s0 = 0, nb = 0, du = 0, misc = 0;
		const uint8_t *fr = nullptr;

		for (uint32_t u0 = tid; u0 < total; u0 += DEPTH * WG) {
			const uint8_t *src[DEPTH];  /* the aligned unit that holds the first byte */
			uint32_t what[DEPTH];       /* shift | two loads << 4 | active << 5 | first byte
						     * << 8 | bytes << 16 | pad << 24 */
			uint32_t to[DEPTH];
			uint4 vl[DEPTH], vh[DEPTH];

#pragma unroll
			for (uint32_t d = 0; d < DEPTH; d++) {
				const uint32_t u = u0 + d * WG;

				what[d] = 0;
				if (u >= total)
					continue;
				if (u >= hi) {      /* left the packet: u < total = start[T] */
					f = find_from(s_start, f, u, T - 1u);
					lo = s_start[f];
					hi = s_start[f + 1u];
					s0 = s_s0[f];
					nb = s_nb[f];
					du = s_du[f];
					misc = s_misc[f];
					fr = frame_at(a, s_off[f], i0 + f);
				}
				const uint32_t k = u - lo, dl = misc & 15u, L0 = misc >> 16;

				if ((misc & M_PATCH) && (k == (L0 + 2u) >> 4 || k == (L0 + 11u) >> 4))
					continue;       /* the patch lane writes it */
				const uint32_t bl = k ? 0u : dl;            /* first byte written */
				const uint32_t e = dl + nb - 16u * k;       /* >= 1: run bytes from the unit's start */
				const uint32_t cnt = min(e, 16u) - bl;
				const uint32_t ss = s0 + 16u * k + bl - dl; /* its source byte */
				const uint32_t sh = ss & 15u;

				src[d] = fr + (ss & ~15u);
				to[d] = du + k;
				what[d] = sh | (sh + cnt > 16u ? 16u : 0u) | 32u | bl << 8 | cnt << 16 |
					((misc & M_PAD) && e <= 16u ? 1u << 24 : 0u);
			}
#pragma unroll
			for (uint32_t d = 0; d < DEPTH; d++) {
				vh[d] = make_uint4(0u, 0u, 0u, 0u);
				if (what[d] & 32u)
					vl[d] = *(const uint4 *)src[d];
				if (what[d] & 16u)
					vh[d] = *(const uint4 *)(src[d] + 16);
			}
#pragma unroll
			for (uint32_t d = 0; d < DEPTH; d++) {
				if (what[d] & 32u) {
					const uint32_t bl = (what[d] >> 8) & 15u;
					uint32_t cnt = (what[d] >> 16) & 31u;
					uint4 v = funnel(vl[d], vh[d], what[d] & 15u);

					if (cnt < 16u)
						v = keep_unit(v, (int32_t)cnt);
					if (what[d] >> 24)
						cnt = 16u - bl;     /* zeros up to align16 */
					if (cnt == 16u)
						dst[to[d]] = v;
					else
						store_bytes((uint8_t *)(dst + to[d]) + bl, v, bl, cnt);
				}
			}
		}
	}

	/* ---- member 0: tot_len, fragment field, checksum ---- */
	if (tid < T && (m_misc & M_PATCH)) {
		const uint8_t *fr = frame_at(a, m_off, i0 + tid);
		const uint32_t L0 = m_misc >> 16, tot = m_hl + m_W;   /* <= 65535 */
		uint32_t sum = 0, fragb = 0;

		for (uint32_t c = 0; c < m_hl; c += 4u) {
			uint32_t w = load32u(fr, L0 + c);

			if (c == 0u)
				w = (w & 0xFFFFu) | (tot & 0xFF00u) << 8 | tot << 24;
			if (c == 4u) {
				w &= 0x00C0FFFFu;       /* DF and the reserved bit stay */
				fragb = w >> 16;
			}
			if (c == 8u)
				w &= 0xFFFFu;
			sum += be_words(w);
		}
		sum = (sum & 0xFFFFu) + (sum >> 16);
		sum = (sum & 0xFFFFu) + (sum >> 16);
		sum = ~sum & 0xFFFFu;
		const uint32_t x[6] = {L0 + 2u, L0 + 3u, L0 + 6u, L0 + 7u, L0 + 10u, L0 + 11u};
		const uint32_t b[6] = {tot >> 8, tot, fragb, 0u, sum >> 8, sum};
		const uint32_t ka = (L0 + 2u) >> 4, kb = (L0 + 11u) >> 4;

		/* both units lie wholly inside member 0's run: L0 + 27 < L0 + tl0 */
		for (uint32_t k = ka; k <= kb; k++) {
			uint4 v = *(const uint4 *)(fr + 16u * k);

#pragma unroll
			for (uint32_t c = 0; c < 6u; c++)
				if (x[c] >> 4 == k)
					put_byte(v, x[c] & 15u, b[c]);
			dst[m_du + k] = v;
		}
	}
}

} /* namespace */

extern "C" int odpg_launch_reass(const odpg_reass_args *a, hipStream_t s)
{
	const uint32_t n = a->src.num;

	if (n) {
		const dim3 per_pkt((n - 1u) / WG + 1u);

		hipLaunchKernelGGL(reass_clear, dim3(std::min((a->tsize - 1u) / WG + 1u, 4096u)), dim3(WG),
				   0, s, *a);
		hipLaunchKernelGGL(reass_key, per_pkt, dim3(WG), 0, s, *a);
		hipLaunchKernelGGL(reass_link, per_pkt, dim3(WG), 0, s, *a);
		hipLaunchKernelGGL(reass_emit, per_pkt, dim3(WG), 0, s, *a);
	}
	/* an empty batch: total and held_offsets only */
	hipLaunchKernelGGL(reass_scan, dim3(1), dim3(SCAN_WG), 0, s, *a);
	if (n) {
		hipLaunchKernelGGL(reass_place, dim3((n - 1u) / WG + 1u), dim3(WG), 0, s, *a);
		hipLaunchKernelGGL(reass_copy, dim3((n - 1u) / T + 1u), dim3(WG), 0, s, *a);
	}
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
