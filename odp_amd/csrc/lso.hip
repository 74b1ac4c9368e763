/* SPDX-License-Identifier: BSD-3-Clause
 *
 * Large-send offload of a device-resident batch (include/odpg_lso.h): the
 * batch form of odp_pktout_send_lso() (odp_packet_io.c:2829-3340). One frame
 * becomes n segments, each the header [0, H) followed by a slice of the
 * payload, with the IPv4 or custom header updates of the profile.
 *
 * Three launches, ordered by the stream alone (no look-back, flags or grid
 * sync between workgroups):
 *   lso_count  a lane per packet, a wave per tile of LSO_TILE = 64 packets:
 *              the rules of _odp_lso_num_packets and the checks that fail a
 *              whole packet, status[i], a 16-byte record per packet in the
 *              plan's `pk` (offset, len, effective P, l3, H, segments,
 *              profile, flags) and per tile the sums of segments and 16-byte
 *              units and the smallest failing index. Profiles sit in LDS.
 *   lso_scan   one workgroup: exclusive scan of the tile sums in place,
 *              total = {segments, 0, first_bad, 0, 16 * units},
 *              seg_first[num].
 *   lso_copy   a workgroup of 256 lanes per tile. Wave 0 scans the tile's 64
 *              records (units, segments, segments of packets with n > 1) into
 *              LDS and stores seg_first[i]; a loop over the tile's positions
 *              writes the descriptors and counts the prefix that fits; then
 *              the two copy phases below.
 *
 * The unit of copying is 16 bytes. Segments of one packet have one size of
 * su = units(H + P) units (the last may be shorter), so inside a packet the
 * segment of a unit is a division (a multiply by the reciprocal of su,
 * corrected by one) and only the packet needs a search.
 *
 * Bulk phase. The tile's destination is one contiguous range of units, lane l
 * of step k owns unit 256 k + l: stores are perfectly coalesced. A lane keeps
 * its packet's [start, end) units and decoded record in registers and searches
 * start[] (LDS, at most 6 steps, forward from the packet it holds) only when
 * its unit leaves that range: per packet boundary, not per unit. Every bulk
 * unit is pure payload or a piece of an unchanged frame: destination unit q
 * of segment k is source bytes [16 q + k P, + 16), at any alignment. It is
 * built from the two aligned 16-byte units around it by a dword select and
 * v_alignbyte_b32; the second is loaded only when bytes of it are needed, so
 * reads stay inside [offset, offset + align16(len)). A lane issues its
 * 2 x LSO_DEPTH loads back to back, then funnels, masks the tail and stores.
 * Units below WIN of a packet with n > 1 are skipped here.
 *
 * Window phase. Everything that is rewritten lies in the first 128 + 8 bytes
 * of a segment, and the unit that holds H mixes header and payload bytes. The
 * first WIN = 9 units of every segment of a packet with n > 1 are built by a
 * group of 16 lanes (9 active) in LDS: header bytes from the aligned source
 * unit, payload bytes through the same funnel. Lane 0 of the group then
 * applies the IPv4 update or the custom fields in profile order on the LDS
 * bytes, so a later field sees an earlier one's write whatever the overlap,
 * and the 9 lanes store the window. 16 segments per round, two barriers per
 * round. The bulk never pays for this: it only skips q < 9.
 *
 * Capacity: a position is written iff its end is <= capacity / 16 and its
 * index < max_segs; both are monotone, so per tile the positions that fit are
 * a prefix of nfit positions ending at unit nuf. The bulk runs over nuf units,
 * the windows over positions below nfit, nfit is added to total->copied (one
 * integer atomic per tile).
 *
 * LDS, bytes: lso_copy 5796 (profiles 1664, records 1024, three scans 780,
 * windows 2304, nfit / nuf 8, padding); lso_count 1664; lso_scan 136.
 * Registers and scratch: DESIGN "Segmentation offload".
 */
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>

#include "lso.h"
#include "unit_copy.h"   /* funnel, keep_unit, scans, find_from */

namespace {

constexpr uint32_t T = LSO_TILE;
constexpr uint32_t WG = 256;
constexpr uint32_t DEPTH = 4;               /* units a lane keeps in flight (two loads each) */
constexpr uint32_t WIN = 9;                 /* units of a segment's patch window: 128 + 8 bytes */
constexpr uint32_t GROUPS = WG / 16;        /* windows per round */
constexpr uint32_t SCAN_WG = 1024;
constexpr uint32_t SAT = 0x7FFFFFFFu;       /* units: beyond capacity / 16 <= 2^28 */
constexpr uint32_t PROF_WORDS = sizeof(odpg_lso_profile_t) / 4u;

static_assert(T == 64, "a tile is one wave of the count pass");
static_assert(sizeof(odpg_lso_profile_t) == 104 && sizeof(odpg_lso_opt_t) == 8 &&
	      sizeof(odpg_lso_pk) == 16, "layout");
static_assert(ODPG_LSO_MAX_PAYLOAD_OFFSET + 8u <= 16u * WIN, "window");

typedef odpg_lso_args Args;

__device__ __forceinline__ void stage_profiles(const Args &a, odpg_lso_profile_t *s_prof)
{
	for (uint32_t w = threadIdx.x; w < a.num_profiles * PROF_WORDS; w += WG)
		((uint32_t *)s_prof)[w] = ((const uint32_t *)a.profiles)[w];
}

/* a packet's record, decoded */
struct Pkt {
	uint32_t off, len, P, l3, H, n, prof, flags;
	uint32_t su;       /* units of a full segment (n > 1) */
	uint32_t lastpay;  /* payload bytes of the last segment (n > 1) */
};

__device__ __forceinline__ Pkt decode(const uint4 r)
{
	Pkt p;

	p.off = r.x;
	p.len = r.y;
	p.P = r.z & 0xFFFFu;
	p.l3 = r.z >> 16;
	p.H = r.w & 0xFFu;
	p.n = (r.w >> 8) & 0xFFu;
	p.prof = (r.w >> 16) & 0xFFu;
	p.flags = r.w >> 24;
	p.su = units_of(p.H + p.P);
	p.lastpay = p.n > 1u ? p.len - p.H - (p.n - 1u) * p.P : 0u;
	return p;
}

__device__ __forceinline__ uint32_t seg_len(const Pkt &p, uint32_t k)
{
	return p.n == 1u ? p.len : p.H + (k + 1u < p.n ? p.P : p.lastpay);
}

__device__ __forceinline__ const uint8_t *frame_of(const Args &a, const Pkt &p, uint32_t i)
{
	return a.src.frames + (a.src.desc ? (uint64_t)p.off : (uint64_t)i * a.src.stride);
}

/* ---- launch 1: the rules per packet, tile sums ----------------------------- */
__global__ __launch_bounds__(WG) void lso_count(Args a)
{
	__shared__ odpg_lso_profile_t s_prof[ODPG_LSO_MAX_PROFILES];
	const uint32_t tid = threadIdx.x, i = blockIdx.x * WG + tid, num = a.src.num;
	uint32_t st = ODPG_LSO_OK, n = 0, flags = 0, bad = 0xFFFFFFFFu;
	uint64_t units = 0;

	stage_profiles(a, s_prof);
	__syncthreads();
	if (i < num) {
		uint2 o;

		if (a.src.opt)
			o = ((const uint2 *)a.src.opt)[i];
		else
			o = make_uint2(a.src.uniform.payload_offset |
				       (uint32_t)a.src.uniform.max_payload_len << 16,
				       a.src.uniform.l3_offset | (uint32_t)a.src.uniform.profile << 16);
		const uint32_t H = o.x & 0xFFFFu, l3 = o.y & 0xFFFFu, prof = (o.y >> 16) & 0xFFu;
		uint32_t P = o.x >> 16, off = 0, len = a.src.stride;

		if (a.src.desc) {
			const uint2 d = ((const uint2 *)a.src.desc)[i];

			off = d.x;
			len = d.y;
		}
		if (prof >= a.num_profiles) {
			st = ODPG_LSO_BAD_PROFILE;
		} else if (H > ODPG_LSO_MAX_PAYLOAD_OFFSET || H > len) {
			st = ODPG_LSO_BAD_OFFSET;
		} else if (H + P > len) {
			n = 1;                    /* no segmentation needed (:3102-3108) */
		} else {
			const odpg_lso_profile_t &pr = s_prof[prof];
			const bool ipv4 = pr.proto == ODPG_LSO_PROTO_IPV4;

			if (ipv4) {
				if (l3 == ODPG_OFFSET_INVALID || H < l3 || H - l3 < 20u)
					st = ODPG_LSO_BAD_L3;
				else
					P = P / 8u * 8u;
			}
			if (st == ODPG_LSO_OK && P == 0u)
				st = ODPG_LSO_BAD_PAYLOAD;
			if (st == ODPG_LSO_OK) {
				const uint32_t pay = len - H;
				const uint32_t left = pay % P;

				n = pay / P + (left != 0u);
				if (n > ODPG_LSO_MAX_SEGMENTS) {
					st = ODPG_LSO_TOO_MANY;
				} else if (n > 1u) {
					const uint32_t lastlen = H + (left ? left : P);

					if (ipv4) {
						/* the aligned word that holds ver_ihl: l3 + 20 <= H <= len */
						const uint8_t *fr = a.src.frames +
							(a.src.desc ? (uint64_t)off : (uint64_t)i * a.src.stride);
						const uint32_t w = *(const uint32_t *)(fr + (l3 & ~3u));

						if (((w >> (8u * (l3 & 3u))) & 0x0Fu) != 5u)
							st = ODPG_LSO_BAD_IHL;
						flags = LSO_PK_PATCH | LSO_PK_IPV4;
					} else {
						for (uint32_t c = 0; c < pr.num_custom; c++)
							if ((uint32_t)pr.field[c].offset + pr.field[c].size > lastlen)
								st = ODPG_LSO_BAD_FIELD;
						flags = pr.num_custom ? LSO_PK_PATCH : 0u;
					}
					units = (uint64_t)(n - 1u) * units_of(H + P) + units_of(lastlen);
				}
			}
		}
		if (st != ODPG_LSO_OK) {
			n = 0;
			units = 0;
			bad = i;
		} else if (n == 1u) {
			units = units_of(len);
		}
		a.dst.status[i] = (uint8_t)st;
		((uint4 *)a.pk)[i] = make_uint4(off, len, (P & 0xFFFFu) | l3 << 16,
						(H & 0xFFu) | n << 8 | prof << 16 | flags << 24);
	}
	uint32_t segs = n;

	for (uint32_t off = 32; off; off >>= 1) {
		segs += __shfl_xor(segs, off);
		units += __shfl_xor(units, off);
		bad = min(bad, (uint32_t)__shfl_xor(bad, off));
	}
	const uint32_t tile = i / T;            /* T == the wave size */

	if ((tid & 63u) == 0 && tile * T < num) {
		a.tsegs[tile] = segs;
		a.tunits[tile] = units;
		a.tbad[tile] = bad;
	}
}

/* ---- launch 2: tile sums -> tile bases, total ------------------------------ */
__global__ __launch_bounds__(SCAN_WG) void lso_scan(Args a)
{
	__shared__ uint64_t s_ws[SCAN_WG / 64];
	__shared__ uint32_t s_bad;
	const uint32_t tid = threadIdx.x, num = a.src.num;
	const uint32_t ntiles = num / T + (num % T != 0);
	uint64_t cu = 0, cs = 0;
	uint32_t bad = 0xFFFFFFFFu;

	if (tid == 0)
		s_bad = 0xFFFFFFFFu;
	for (uint32_t base = 0; base < ntiles; base += SCAN_WG) {
		const uint32_t t = base + tid;
		const uint64_t vu = t < ntiles ? a.tunits[t] : 0u, vs = t < ntiles ? a.tsegs[t] : 0u;
		uint64_t au, as;
		const uint64_t bu = block_excl_scan<SCAN_WG / 64>(vu, s_ws, &au);
		const uint64_t bs = block_excl_scan<SCAN_WG / 64>(vs, s_ws, &as);

		if (t < ntiles) {
			a.tunits[t] = cu + bu;
			a.tsegs[t] = (uint32_t)(cs + bs);     /* num <= 2^25: below 2^31 */
			bad = min(bad, a.tbad[t]);
		}
		cu += au;
		cs += as;
	}
	__syncthreads();
	if (bad != 0xFFFFFFFFu)
		atomicMin(&s_bad, bad);
	__syncthreads();
	if (tid == 0) {
		a.dst.total->num_segs = (uint32_t)cs;
		a.dst.total->copied = 0;         /* lso_copy adds each tile's share */
		a.dst.total->first_bad = min(s_bad, num);
		a.dst.total->reserved = 0;
		a.dst.total->bytes = cu << 4;
		a.dst.seg_first[num] = (uint32_t)cs;
	}
}

/* ---- launch 3: descriptors, bulk units, patch windows ---------------------- */
__device__ void patch_ipv4(uint8_t *b, const Pkt &p, uint32_t k, uint32_t seglen)
{
	uint8_t *ip = b + p.l3;
	const uint32_t tot = seglen - p.l3;
	uint32_t frag = ((uint32_t)ip[6] << 8 | ip[7]) + ((k * p.P) >> 3), sum = 0;

	if (k + 1u < p.n)
		frag |= 0x2000u;
	ip[2] = (uint8_t)(tot >> 8);
	ip[3] = (uint8_t)tot;
	ip[6] = (uint8_t)(frag >> 8);
	ip[7] = (uint8_t)frag;
	ip[10] = 0;
	ip[11] = 0;
	for (uint32_t c = 0; c < 20u; c += 2u)
		sum += (uint32_t)ip[c] << 8 | ip[c + 1u];
	sum = (sum & 0xFFFFu) + (sum >> 16);
	sum = (sum & 0xFFFFu) + (sum >> 16);
	sum = ~sum;
	ip[10] = (uint8_t)(sum >> 8);
	ip[11] = (uint8_t)sum;
}

__device__ void patch_custom(uint8_t *b, const odpg_lso_profile_t &pr, const Pkt &p, uint32_t k)
{
	for (uint32_t c = 0; c < pr.num_custom; c++) {
		const odpg_lso_field_t &f = pr.field[c];
		uint8_t *q = b + f.offset;
		const uint32_t size = f.size;

		if (f.mod_op == ODPG_LSO_ADD_SEGMENT_NUM) {
			uint64_t v = 0;

			for (uint32_t e = 0; e < size; e++)
				v = v << 8 | q[e];
			v += k;
			for (uint32_t e = 0; e < size; e++)
				q[size - 1u - e] = (uint8_t)(v >> (8u * e));
		} else {
			const odpg_lso_bits_t w = k == 0 ? f.first : k + 1u == p.n ? f.last : f.middle;

			q[0] = (uint8_t)((q[0] & ~w.mask) | (w.value & w.mask));
		}
	}
}

__global__ __launch_bounds__(WG) void lso_copy(Args a)
{
	__shared__ odpg_lso_profile_t s_prof[ODPG_LSO_MAX_PROFILES];
	__shared__ uint4 s_pk[T];
	__shared__ uint32_t s_ustart[T + 1];   /* tile-relative units, saturating */
	__shared__ uint32_t s_sfirst[T + 1];   /* tile-relative positions */
	__shared__ uint32_t s_wfirst[T + 1];   /* likewise, packets with n > 1 only */
	__shared__ uint4 s_win[GROUPS][WIN];
	__shared__ uint32_t s_nfit, s_nuf;
	const uint32_t tid = threadIdx.x, i0 = blockIdx.x * T, num = a.src.num;
	const uint64_t G = a.tunits[blockIdx.x], capu = a.dst.capacity >> 4;
	const uint32_t S = a.tsegs[blockIdx.x];

	stage_profiles(a, s_prof);
	if (tid == 0) {
		s_nfit = 0;
		s_nuf = 0;
	}
	if (tid < T) {
		const uint32_t i = i0 + tid;
		const uint4 r = i < num ? ((const uint4 *)a.pk)[i] : make_uint4(0u, 0u, 0u, 0u);
		const Pkt p = decode(r);
		const uint64_t units = p.n == 1u ? units_of(p.len)
			: p.n ? (uint64_t)(p.n - 1u) * p.su + units_of(p.H + p.lastpay) : 0u;
		const uint64_t iu = wave_incl_scan(units);
		const uint32_t is = wave_incl_scan(p.n), iw = wave_incl_scan(p.n > 1u ? p.n : 0u);

		s_pk[tid] = r;
		s_ustart[tid] = (uint32_t)min(iu - units, (uint64_t)SAT);
		s_sfirst[tid] = is - p.n;
		s_wfirst[tid] = iw - (p.n > 1u ? p.n : 0u);
		if (tid == T - 1u) {
			s_ustart[T] = (uint32_t)min(iu, (uint64_t)SAT);
			s_sfirst[T] = is;
			s_wfirst[T] = iw;
		}
		if (i < num)
			a.dst.seg_first[i] = S + is - p.n;
	}
	__syncthreads();
	const uint32_t nseg = s_sfirst[T], nw = s_wfirst[T];

	/* descriptors per position; the positions that fit are a prefix */
	for (uint32_t r0 = 0; r0 < nseg; r0 += WG) {
		const uint32_t r = r0 + tid;
		bool fits = false;

		if (r < nseg) {
			const uint32_t f = find_from(s_sfirst, 0u, r, T - 1u), k = r - s_sfirst[f];
			const Pkt p = decode(s_pk[f]);
			const uint32_t seglen = seg_len(p, k), j = S + r;
			const uint64_t start = (uint64_t)s_ustart[f] + (uint64_t)k * p.su;
			const uint64_t end = start + units_of(seglen);

			fits = j < a.dst.max_segs && G + end <= capu;
			/* a written segment ends at or below 2^32 */
			if (j < a.dst.max_segs)
				((uint2 *)a.dst.desc)[j] = fits ? make_uint2((uint32_t)((G + start) << 4), seglen)
								: make_uint2(0u, 0u);
			if (fits)
				atomicMax(&s_nuf, (uint32_t)end);
		}
		const uint32_t c = (uint32_t)__popcll(__ballot(fits));

		if ((tid & 63u) == 0 && c)
			atomicAdd(&s_nfit, c);
	}
	__syncthreads();
	const uint32_t nfit = s_nfit, nuf = s_nuf;   /* nuf <= capu - G <= 2^28 */

	if (tid == 0 && nfit)
		atomicAdd(&a.dst.total->copied, nfit);
	uint4 *dst = (uint4 *)a.dst.frames + G;

	/* ---- bulk ---- */
	{
		uint32_t f = 0, lo = 0, hi = 0;     /* the lane's packet: units [lo, hi) */
		Pkt p = {};
		const uint8_t *fr = nullptr;
		float rcp = 0.f;

		for (uint32_t u0 = tid; u0 < nuf; u0 += DEPTH * WG) {
			const uint8_t *src[DEPTH];  /* the aligned unit that holds the first byte */
			uint32_t sh[DEPTH];         /* shift | two loads << 4 | active << 5 */
			uint32_t left[DEPTH];
			uint4 vl[DEPTH], vh[DEPTH];

#pragma unroll
			for (uint32_t d = 0; d < DEPTH; d++) {
				const uint32_t u = u0 + d * WG;

				sh[d] = 0;
				if (u >= nuf)
					continue;
				if (u >= hi) {      /* left the packet: u < nuf <= start[T] */
					f = find_from(s_ustart, f, u, T - 1u);
					lo = s_ustart[f];
					hi = s_ustart[f + 1u];
					p = decode(s_pk[f]);
					fr = frame_of(a, p, i0 + f);
					rcp = __frcp_rn((float)p.su);
				}
				uint32_t q = u - lo, k = 0;

				if (p.n > 1u) {     /* q < 64 * 4104: exact as a float */
					k = (uint32_t)((float)q * rcp);
					q -= k * p.su;
					if ((int32_t)q < 0) {
						k--;
						q += p.su;
					} else if (q >= p.su) {
						k++;
						q -= p.su;
					}
					if (q < WIN)
						continue;       /* the window phase writes it */
				}
				const uint32_t s = 16u * q + k * p.P;   /* n == 1: 16 q < len */
				const uint32_t v = seg_len(p, k) - 16u * q;   /* >= 1 */

				left[d] = v;
				src[d] = fr + (s & ~15u);
				sh[d] = (s & 15u) | ((s & 15u) + min(v, 16u) > 16u ? 16u : 0u) | 32u;
			}
#pragma unroll
			for (uint32_t d = 0; d < DEPTH; d++) {
				vh[d] = make_uint4(0u, 0u, 0u, 0u);
				if (sh[d] & 32u)
					vl[d] = *(const uint4 *)src[d];
				if (sh[d] & 16u)
					vh[d] = *(const uint4 *)(src[d] + 16);
			}
#pragma unroll
			for (uint32_t d = 0; d < DEPTH; d++) {
				if (sh[d] & 32u) {
					uint4 v = funnel(vl[d], vh[d], sh[d] & 15u);

					if (left[d] < 16u)
						v = keep_unit(v, (int32_t)left[d]);
					dst[u0 + d * WG] = v;
				}
			}
		}
	}

	/* ---- windows: 16 lanes per segment of a packet with n > 1 ---- */
	const uint32_t g = tid >> 4, l = tid & 15u;

	for (uint32_t wb = 0; wb < nw; wb += GROUPS) {
		const uint32_t w = wb + g;
		bool act = false, has = false;
		uint32_t f = 0, k = 0, seglen = 0;
		Pkt p = {};

		if (w < nw) {
			f = find_from(s_wfirst, 0u, w, T - 1u);
			k = w - s_wfirst[f];
			act = s_sfirst[f] + k < nfit;
		}
		if (act) {
			p = decode(s_pk[f]);
			seglen = seg_len(p, k);
			has = l < WIN && 16u * l < seglen;
		}
		if (has) {
			const uint8_t *fr = frame_of(a, p, i0 + f);
			const uint32_t d = 16u * l, s = d + k * p.P, shift = s & 15u;
			/* destination bytes [b0, b1) of the unit are payload */
			const uint32_t b0 = p.H > d ? p.H - d : 0u, b1 = min(16u, seglen - d);
			const bool pay = b0 < b1;
			uint4 hd = make_uint4(0u, 0u, 0u, 0u), vl = hd, vh = hd;

			if (d < p.H)
				hd = *(const uint4 *)(fr + d);
			if (pay && b0 < 16u - shift)
				vl = *(const uint4 *)(fr + (s & ~15u));
			if (pay && b1 > 16u - shift)
				vh = *(const uint4 *)(fr + (s & ~15u) + 16);
			const uint4 pv = funnel(vl, vh, shift);
			const int32_t hb = (int32_t)p.H - (int32_t)d;   /* header bytes of the unit */
			uint4 v;

			v.x = keep_bytes(hd.x, hb) | (pv.x ^ keep_bytes(pv.x, hb));
			v.y = keep_bytes(hd.y, hb - 4) | (pv.y ^ keep_bytes(pv.y, hb - 4));
			v.z = keep_bytes(hd.z, hb - 8) | (pv.z ^ keep_bytes(pv.z, hb - 8));
			v.w = keep_bytes(hd.w, hb - 12) | (pv.w ^ keep_bytes(pv.w, hb - 12));
			s_win[g][l] = keep_unit(v, (int32_t)min(16u, seglen - d));
		}
		__syncthreads();
		if (act && l == 0 && (p.flags & LSO_PK_PATCH)) {
			if (p.flags & LSO_PK_IPV4)
				patch_ipv4((uint8_t *)s_win[g], p, k, seglen);
			else
				patch_custom((uint8_t *)s_win[g], s_prof[p.prof], p, k);
		}
		__syncthreads();
		if (has)
			dst[s_ustart[f] + k * p.su + l] = s_win[g][l];
	}
}

} /* namespace */

extern "C" int odpg_launch_lso(const odpg_lso_args *a, hipStream_t s)
{
	const uint32_t n = a->src.num;

	if (n)
		hipLaunchKernelGGL(lso_count, dim3((n - 1u) / WG + 1u), dim3(WG), 0, s, *a);
	/* an empty batch: seg_first[0] and total only */
	hipLaunchKernelGGL(lso_scan, dim3(1), dim3(SCAN_WG), 0, s, *a);
	if (n)
		hipLaunchKernelGGL(lso_copy, dim3((n - 1u) / T + 1u), dim3(WG), 0, s, *a);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
