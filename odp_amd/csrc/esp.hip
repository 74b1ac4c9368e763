/* SPDX-License-Identifier: BSD-3-Clause
 *
 * ESP tunnel-mode AES-GCM of a device-resident batch (include/odpg_esp.h): the
 * batch form of the reference's ipsec_out_esp / ipsec_in_esp paths
 * (odp_ipsec.c). The first kernel family here that is bound by arithmetic:
 * per 16 bytes one AES encryption (10 to 14 rounds of four table lookups per
 * word) and one multiplication in GF(2^128).
 *
 * Launches, ordered by the stream alone (no kernel waits for another lane,
 * wave or workgroup; every loop is bounded by a frame or batch size):
 *   esp_prep    a lane per packet, a workgroup per 256: the header's
 *               per-packet rules up to the point where crypto starts, status,
 *               a 16-byte record, the bytes the packet reserves in the output,
 *               the partition key (outbound: the SA, max_sas for a failed
 *               packet), inbound seq[i]; per workgroup the sums of 16-byte
 *               units and OK packets and the smallest failing index.
 *   dlv_*       outbound: the stable radix partition of the packet indices by
 *               SA (radix_pass.h, three launches up to 2047 SAs). A packet's
 *               rank among the OK packets of its SA is its position in `order`
 *               minus offsets[sa]: the partition is stable.
 *   esp_seq     outbound, a lane per position of `order`: seq64 = next_seq[sa]
 *               + rank, seq[i] its low word.
 *   esp_advance outbound, a lane per SA: next_seq[sa] += its bucket's size. A
 *               launch of its own, so every read of next_seq precedes it.
 *   esp_scan    one workgroup: exclusive scan of the tile sums in place, total.
 *   esp_place   a lane per packet: the packet's first output unit (block scan
 *               plus the tile's base), whether it fits, desc[i], copied.
 *   esp_crypt   the hot path, below.
 *
 * esp_crypt. Work is split by 16-byte block, not by packet: a group of 16
 * lanes owns a packet, a workgroup of 256 lanes 16 packets (ODPG_ESP_TILE), and
 * a packet's blocks are taken in chunks of 16, lane l the chunk's l-th. The
 * blocks are "virtual": v = 0 is the AAD block, whose lane also encrypts J0
 * (counter 1) for the tag, v = 1 .. nb the cipher blocks (counter v + 1), v =
 * nb + 1 the length block. So a 64-byte inner packet (5 cipher blocks) keeps 7
 * lanes busy in its one chunk, a 1500-byte one 16 lanes in 6 chunks.
 *
 *   AES      one 1 KiB T-table in LDS (built by the host, copied once per
 *            workgroup), the three others by rotation; the last round takes
 *            S[x] from the table's second byte. Round keys of the group's SA
 *            (240 B) sit in the group's LDS slice.
 *   GHASH    lane l multiplies its block (lane 0: XORed with the running
 *            value Y) by H^(k - l), k the blocks of the chunk; the group
 *            XOR-reduces over four butterfly steps and the sum is the new Y:
 *            Horner in steps of H^k. H^1 .. H^16 of the SA (256 B, made on the
 *            host) sit beside the round keys. gfx950 has no carry-less
 *            multiply: the product is bit-serial, both operands in registers
 *            (esp.h), 128 steps of 14 integer operations.
 *   Source   bytes at any alignment: whole aligned 16-byte units inside the
 *            frame, realigned through lso.hip's byte funnel (unit_copy.h); the
 *            second unit is loaded only when bytes of it are needed.
 *   Output   built in a 512-byte ring per group in LDS at its destination
 *            alignment: the bytes of fr[0, L) that share a unit with what
 *            follows, the outer IPv4, ESP header and IV (lane 0), a block per
 *            lane, the ICV (lane 0, the one that holds E(J0)), zeros up to the
 *            16-byte boundary. After every chunk the units that are complete
 *            leave as whole 16-byte stores, a unit per lane: every unit of a
 *            frame is written exactly once. Units wholly inside fr[0, L) go
 *            from source to destination without the ring.
 *   Inbound  two passes over the ciphertext, so that a frame that fails is
 *            written nowhere: GHASH alone and the tag compare; the trailer
 *            (the block or two that hold pad length and next header, then the
 *            blocks that hold pad bytes); then decryption into the ring. The
 *            second read of the ciphertext hits L2.
 *
 * Lanes of a group run in one wave: LDS traffic between them is ordered by a
 * wavefront fence, no workgroup barrier after the staging one.
 *
 * LDS of esp_crypt, bytes: T-table 1024, SA slices 16 x 496 = 7936, rings
 * 16 x 512 = 8192: 17152. esp_prep 48, esp_scan 136, esp_place 32.
 */
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>

#include "esp.h"
#include "unit_copy.h"   /* funnel, keep_unit, scans */
#include "radix_pass.h"

namespace {

constexpr uint32_t G = ESP_GROUP;
constexpr uint32_t T = ESP_TILE;
constexpr uint32_t WG = T * G;              /* esp_crypt */
constexpr uint32_t PWG = ESP_PREP_WG;       /* esp_prep, esp_place, esp_seq */
constexpr uint32_t SCAN_WG = 1024;
constexpr uint32_t RING = 512;              /* bytes; a power of two */
constexpr uint32_t NONE = 0xFFFFFFFFu;

static_assert(WG == 256 && G == 16 && 64 % G == 0, "a group is a quarter of a wave");
static_assert(sizeof(odpg_esp_rec) == 16 && sizeof(odpg_esp_sa_dev) == 4 * (ESP_SA_LDS_WORDS + 8),
	      "layout");
/* a group's ring holds what is not flushed yet: below a unit, the up to 15 + 36
 * bytes in front of the first block, a chunk and the ICV */
static_assert(16u + 51u + 16u * G + 16u <= RING, "ring");

typedef odpg_esp_args Args;

/* partition source: the SA of an OK packet, max_sas otherwise */
struct Keys {
	const uint32_t *src;
	uint32_t num;
	uint32_t max_sas;

	__device__ __forceinline__ uint32_t key(uint32_t w) const
	{
		return min(w, max_sas);
	}
};

__device__ __forceinline__ void wave_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint32_t bswap(uint32_t v)
{
	return __builtin_bswap32(v);
}

__device__ __forceinline__ uint32_t be16(const uint8_t *p)
{
	return (uint32_t)p[0] << 8 | p[1];
}

__device__ __forceinline__ uint32_t be32(const uint8_t *p)
{
	return be16(p) << 16 | be16(p + 2);
}

/* bytes [0, nb) of the frame bytes at p, nb in [1, 16], as little-endian words,
 * zero beyond nb: the aligned unit that holds p[0], and the next one only if
 * bytes of it are wanted */
__device__ __forceinline__ uint4 load_bytes(const uint8_t *p, uint32_t nb)
{
	const uint32_t sh = (uint32_t)(uintptr_t)p & 15u;
	const uint4 *u = (const uint4 *)(p - sh);
	const uint4 lo = u[0];
	uint4 hi = make_uint4(0u, 0u, 0u, 0u);

	if (sh + nb > 16u)
		hi = u[1];
	return keep_unit(funnel(lo, hi, sh), (int32_t)nb);
}

/* ---- launch 1: the rules per packet, tile sums ----------------------------- */
template <bool OUT>
__global__ __launch_bounds__(PWG) void esp_prep(Args a)
{
	__shared__ uint64_t s_units[PWG / 64];
	__shared__ uint32_t s_ok[PWG / 64], s_bad[PWG / 64];
	const uint32_t tid = threadIdx.x, i = blockIdx.x * PWG + tid, num = a.src.num;
	uint64_t units = 0;
	uint32_t ok = 0, bad = NONE;

	if (i < num) {
		uint32_t off = 0, n = a.src.stride;

		if (a.src.desc) {
			const uint2 d = ((const uint2 *)a.src.desc)[i];

			off = d.x;
			n = d.y;
		}
		const uint8_t *fr = a.src.frames + (a.src.desc ? (uint64_t)off : (uint64_t)i * a.src.stride);
		const uint32_t s = a.src.sa ? a.src.sa[i] : a.src.uniform_sa;
		const uint32_t L = a.src.l3_offset ? a.src.l3_offset[i] : a.src.uniform_l3;
		uint32_t st = ODPG_ESP_OK, ilen = 0, misc = 0, fl = 0, olen = 0, seq = 0;

		if (s >= a.max_sas || !(a.sas[s].flags & ESP_SA_VALID)) {
			st = ODPG_ESP_NO_SA;
		} else if (L + 20u > n) {
			st = ODPG_ESP_BAD_L3;
		} else if (OUT) {
			const uint32_t b0 = fr[L], ver = b0 >> 4;

			if (ver == 4u) {
				ilen = be16(fr + L + 2u);
				misc = fr[L + 1u];
				fl = (fr[L + 6u] & 0x40u) ? ESP_REC_DF : 0u;
				if ((b0 & 15u) < 5u || ilen < 4u * (b0 & 15u))
					st = ODPG_ESP_BAD_L3;
			} else if (ver == 6u && L + 40u <= n) {
				ilen = 40u + be16(fr + L + 4u);
				misc = (b0 & 15u) << 4 | fr[L + 1u] >> 4;
				fl = ESP_REC_V6;
			} else {
				st = ODPG_ESP_BAD_L3;
			}
			if (st == ODPG_ESP_OK && L + ilen > n)
				st = ODPG_ESP_BAD_L3;
			if (st == ODPG_ESP_OK) {
				const uint32_t tot = 52u + ((ilen + 5u) & ~3u);

				if (tot > a.sas[s].mtu)
					st = ODPG_ESP_MTU;
				olen = L + tot;
			}
		} else {
			const uint32_t b0 = fr[L], ihl = b0 & 15u, tot = be16(fr + L + 2u);

			if ((b0 >> 4) != 4u || ihl < 5u || (be16(fr + L + 6u) & 0x3FFFu) || tot > n - L) {
				st = ODPG_ESP_BAD_L3;
			} else if (fr[L + 9u] != 50u) {
				st = ODPG_ESP_BAD_PROTO;
			} else if (tot < 4u * ihl + 34u) {
				st = ODPG_ESP_BAD_LEN;
			} else {
				seq = be32(fr + L + 4u * ihl + 4u);
				if (be32(fr + L + 4u * ihl) != a.sas[s].spi)
					st = ODPG_ESP_BAD_SPI;
				ilen = tot - 4u * ihl - 32u;
				misc = ihl;
				olen = L + ilen - 2u;
			}
		}
		if (st != ODPG_ESP_OK) {
			olen = 0;
			bad = i;
		} else {
			ok = 1;
			units = units_of(olen);
		}
		a.dst.status[i] = (uint8_t)st;
		a.dst.seq[i] = seq;
		if (OUT)
			a.skey[i] = st == ODPG_ESP_OK ? s : a.max_sas;
		((uint4 *)a.rec)[i] = make_uint4(off, (L & 0xFFFFu) | ilen << 16,
						 (s & 0xFFFFu) | st << 16 | misc << 24, olen | fl << 24);
	}
	for (uint32_t o = 32; o; o >>= 1) {
		units += __shfl_xor(units, o);
		ok += __shfl_xor(ok, o);
		bad = min(bad, (uint32_t)__shfl_xor(bad, o));
	}
	if ((tid & 63u) == 0) {
		s_units[tid >> 6] = units;
		s_ok[tid >> 6] = ok;
		s_bad[tid >> 6] = bad;
	}
	__syncthreads();
	if (tid == 0) {
		for (uint32_t w = 1; w < PWG / 64; w++) {
			units += s_units[w];
			ok += s_ok[w];
			bad = min(bad, s_bad[w]);
		}
		a.tunits[blockIdx.x] = units;
		a.tok[blockIdx.x] = ok;
		a.tbad[blockIdx.x] = bad;
	}
}

/* ---- outbound: sequence numbers from the partition -------------------------- */
__global__ __launch_bounds__(PWG) void esp_seq(Args a)
{
	const uint32_t m = blockIdx.x * PWG + threadIdx.x;

	if (m >= a.src.num)
		return;
	const uint32_t i = a.order[m];

	if (i >= a.src.num)     /* cannot happen: `order` is a permutation */
		return;
	const uint32_t s = a.skey[i];

	if (s < a.max_sas) {
		const uint64_t q = a.next_seq[s] + (m - a.offsets[s]);

		a.seq64[i] = q;
		a.dst.seq[i] = (uint32_t)q;
	}
}

__global__ __launch_bounds__(PWG) void esp_advance(Args a)
{
	const uint32_t s = blockIdx.x * PWG + threadIdx.x;

	if (s < a.max_sas) {
		const uint32_t c = a.offsets[s + 1u] - a.offsets[s];

		if (c && c <= a.src.num)
			a.next_seq[s] += c;
	}
}

/* ---- tile sums -> tile bases, total ------------------------------------------ */
__global__ __launch_bounds__(SCAN_WG) void esp_scan(Args a)
{
	__shared__ uint64_t s_ws[SCAN_WG / 64];
	__shared__ uint32_t s_bad, s_ok;
	const uint32_t tid = threadIdx.x, num = a.src.num;
	const uint32_t ntiles = num / PWG + (num % PWG != 0);
	uint64_t cu = 0;
	uint32_t bad = NONE, ok = 0;

	if (tid == 0) {
		s_bad = NONE;
		s_ok = 0;
	}
	for (uint32_t base = 0; base < ntiles; base += SCAN_WG) {
		const uint32_t t = base + tid;
		const uint64_t vu = t < ntiles ? a.tunits[t] : 0u;
		uint64_t au;
		const uint64_t bu = block_excl_scan<SCAN_WG / 64>(vu, s_ws, &au);

		if (t < ntiles) {
			a.tunits[t] = cu + bu;
			bad = min(bad, a.tbad[t]);
			ok += a.tok[t];
		}
		cu += au;
	}
	__syncthreads();
	if (bad != NONE)
		atomicMin(&s_bad, bad);
	if (ok)
		atomicAdd(&s_ok, ok);
	__syncthreads();
	if (tid == 0) {
		a.dst.total->num_out = s_ok;       /* inbound: esp_crypt takes its failures off */
		a.dst.total->copied = 0;           /* esp_place adds each tile's share */
		a.dst.total->first_bad = min(s_bad, num);
		a.dst.total->reserved = 0;
		a.dst.total->bytes = cu << 4;
	}
}

/* ---- output positions, descriptors, copied ------------------------------------ */
__global__ __launch_bounds__(PWG) void esp_place(Args a)
{
	__shared__ uint64_t s_ws[PWG / 64];
	const uint32_t tid = threadIdx.x, i = blockIdx.x * PWG + tid, num = a.src.num;
	const uint64_t capu = a.dst.capacity >> 4;
	uint4 r = make_uint4(0u, 0u, 0u, 0u);
	uint64_t all;

	if (i < num)
		r = ((const uint4 *)a.rec)[i];
	const uint32_t olen = r.w & 0xFFFFFFu, st = (r.z >> 16) & 0xFFu;
	const uint64_t units = units_of(olen);
	const uint64_t start = a.tunits[blockIdx.x] + block_excl_scan<PWG / 64>(units, s_ws, &all);
	const bool fits = i < num && i < a.dst.max_out && start + units <= capu;

	if (i < num) {
		/* a position that fits ends at or below 2^32 bytes: start < 2^28 */
		a.ounit[i] = fits ? (uint32_t)start : ESP_NOFIT;
		if (i < a.dst.max_out)
			((uint2 *)a.dst.desc)[i] = fits ? make_uint2((uint32_t)(start << 4),
								     st == ODPG_ESP_OK ? olen : 0u)
							: make_uint2(0u, 0u);
	}
	const uint32_t c = (uint32_t)__popcll(__ballot(fits));

	if ((tid & 63u) == 0 && c)
		atomicAdd(&a.dst.total->copied, c);
}

/* ---- the hot path --------------------------------------------------------------- */

/* a group's view of its packet's output: the ring and what has left it */
struct Out {
	uint8_t *ring;      /* the group's RING bytes of LDS */
	uint4 *dst;         /* the frame's first unit */
	uint32_t base0;     /* ring byte 0 is frame byte base0, a multiple of 16 */
	uint32_t fu;        /* units below this one are stored */
	uint32_t l;         /* lane of the group */

	__device__ __forceinline__ void put(uint32_t pos, uint32_t byte)
	{
		ring[(pos - base0) & (RING - 1u)] = (uint8_t)byte;
	}

	/* nb bytes of the little-endian words v at frame byte pos */
	__device__ __forceinline__ void put_block(uint32_t pos, uint4 v, uint32_t nb)
	{
		const uint32_t w[4] = {v.x, v.y, v.z, v.w};

#pragma unroll
		for (uint32_t k = 0; k < 16u; k++)
			if (k < nb)
				put(pos + k, w[k >> 2] >> (8u * (k & 3u)));
	}

	/* every unit that ends at or below frame byte `end` leaves the ring */
	__device__ __forceinline__ void flush(uint32_t end)
	{
		const uint32_t uc = end >> 4;

		wave_sync();
		for (uint32_t u = fu + l; u < uc; u += G)
			dst[u] = *(const uint4 *)(ring + (((u << 4) - base0) & (RING - 1u)));
		wave_sync();
		fu = max(fu, uc);
	}
};

/* XOR of z over the group's lanes, in every lane */
__device__ __forceinline__ void group_xor(uint32_t z[4])
{
#pragma unroll
	for (uint32_t o = G / 2u; o; o >>= 1) {
#pragma unroll
		for (uint32_t w = 0; w < 4u; w++)
			z[w] ^= __shfl_xor(z[w], o, G);
	}
}

/* one chunk of GHASH: lane l < k holds block x; y <- (y ^ x_0) H^k ^ x_1 H^(k-1) ^ .. */
__device__ __forceinline__ void ghash_chunk(const uint32_t *hpow, uint32_t l, uint32_t k,
					    uint32_t x[4], uint32_t y[4])
{
	uint32_t z[4] = {0u, 0u, 0u, 0u};
	const bool on = l < k;
	const uint32_t *h = hpow + 4u * (on ? k - l - 1u : 0u);
	const uint32_t hp[4] = {h[0], h[1], h[2], h[3]};

	if (l == 0) {
		x[0] ^= y[0];
		x[1] ^= y[1];
		x[2] ^= y[2];
		x[3] ^= y[3];
	}
	esp_gf_mul(x, hp, z);
	if (!on)
		z[0] = z[1] = z[2] = z[3] = 0;
	group_xor(z);
	y[0] = z[0];
	y[1] = z[1];
	y[2] = z[2];
	y[3] = z[3];
}

/* the keystream block of counter ctr, as little-endian words to XOR onto data */
__device__ __forceinline__ uint4 keystream(const uint32_t *rk, uint32_t nr, const uint32_t *te0,
					   uint32_t salt, uint32_t iv0, uint32_t iv1, uint32_t ctr)
{
	uint32_t s[4] = {salt, iv0, iv1, ctr};

	esp_aes_encrypt(rk, nr, te0, s);
	return make_uint4(bswap(s[0]), bswap(s[1]), bswap(s[2]), bswap(s[3]));
}

__device__ __forceinline__ uint32_t byte_of(uint4 v, uint32_t k)
{
	const uint32_t w = k < 4u ? v.x : k < 8u ? v.y : k < 12u ? v.z : v.w;

	return (w >> (8u * (k & 3u))) & 0xFFu;
}

template <bool OUT>
__global__ __launch_bounds__(WG) void esp_crypt(Args a)
{
	__shared__ uint32_t s_te[256];
	__shared__ uint32_t s_sa[T][ESP_SA_LDS_WORDS];
	__shared__ __attribute__((aligned(16))) uint8_t s_ring[T][RING];
	const uint32_t tid = threadIdx.x, g = tid / G, l = tid % G;
	const uint32_t i = blockIdx.x * T + g, num = a.src.num;
	uint4 r = make_uint4(0u, 0u, 0u, 0u);
	uint32_t ou = ESP_NOFIT;
	bool act = false;

	s_te[tid] = a.te0[tid];
	if (i < num) {
		r = ((const uint4 *)a.rec)[i];
		ou = a.ounit[i];
		/* an inbound packet that does not fit is still authenticated */
		act = ((r.z >> 16) & 0xFFu) == ODPG_ESP_OK && (!OUT || ou != ESP_NOFIT);
	}
	const uint32_t sa = r.z & 0xFFFFu;
	const odpg_esp_sa_dev *sad = a.sas + (act ? sa : 0u);

	if (act)
		for (uint32_t w = l; w < ESP_SA_LDS_WORDS; w += G)
			s_sa[g][w] = ((const uint32_t *)sad)[w];
	__syncthreads();
	if (!act)
		return;

	const uint32_t *rk = s_sa[g], *hpow = s_sa[g] + 60;
	const uint32_t nr = sad->nr, salt = sad->salt;
	const uint32_t L = r.y & 0xFFFFu, ilen = r.y >> 16, misc = r.z >> 24, fl = r.w >> 24;
	const uint8_t *fr = a.src.frames + (a.src.desc ? (uint64_t)r.x : (uint64_t)i * a.src.stride);
	const bool fits = ou != ESP_NOFIT;
	Out o = {s_ring[g], (uint4 *)a.dst.frames + (fits ? ou : 0u), L & ~15u, 0u, l};
	uint32_t y[4] = {0u, 0u, 0u, 0u}, ej0[4] = {0u, 0u, 0u, 0u};

	if (fits) {
		/* fr[0, L): whole units straight across, the rest into the ring */
		for (uint32_t u = l; u < (L >> 4); u += G)
			o.dst[u] = load_bytes(fr + 16u * u, 16u);
		o.fu = L >> 4;
		if (l == 0 && (L & 15u))
			o.put_block(o.base0, load_bytes(fr + o.base0, L & 15u), L & 15u);
	}

	if (OUT) {
		const uint32_t E = (ilen + 5u) & ~3u, nb = (E + 15u) >> 4, N = nb + 2u;
		const uint32_t pad = E - ilen - 2u, next = (fl & ESP_REC_V6) ? 41u : 4u;
		const uint32_t p0 = L + 36u, tot = 52u + E;
		const uint64_t q64 = a.seq64[i];
		const uint32_t seq = (uint32_t)q64;
		/* the IV is seq64's little-endian bytes: as big-endian words */
		const uint32_t iv0 = bswap(seq), iv1 = bswap((uint32_t)(q64 >> 32));

		if (l == 0) {
			const uint32_t tos = misc, sfl = sad->flags;
			const uint32_t tos2 = (sfl & ESP_SA_COPY_DSCP) ? tos
					    : (tos & 3u) | ((sad->ttl_dscp >> 8) & 0x3Fu) << 2;
			const bool df = (sfl & ESP_SA_COPY_DF) ? (fl & ESP_REC_DF) : (sfl & ESP_SA_DF);
			const uint32_t frag = df ? 0x4000u : 0u, idv = frag ? 0u : seq & 0xFFFFu;
			uint32_t h[9], sum;   /* big-endian words */

			h[0] = 0x45000000u | tos2 << 16 | tot;
			h[1] = idv << 16 | frag;
			h[2] = (sad->ttl_dscp & 0xFFu) << 24 | 50u << 16;
			h[3] = sad->tun_src;
			h[4] = sad->tun_dst;
			sum = (h[0] >> 16) + (h[0] & 0xFFFFu) + (h[1] >> 16) + (h[1] & 0xFFFFu) +
			      (h[2] >> 16) + (h[3] >> 16) + (h[3] & 0xFFFFu) + (h[4] >> 16) +
			      (h[4] & 0xFFFFu);
			sum = (sum & 0xFFFFu) + (sum >> 16);
			sum = (sum & 0xFFFFu) + (sum >> 16);
			h[2] |= ~sum & 0xFFFFu;
			h[5] = sad->spi;
			h[6] = seq;
			h[7] = iv0;
			h[8] = iv1;
			for (uint32_t k = 0; k < 36u; k++)
				o.put(L + k, h[k >> 2] >> (24u - 8u * (k & 3u)));
		}
		for (uint32_t c = 0; c * G < N; c++) {
			const uint32_t v = c * G + l, k = min(G, N - c * G);
			uint32_t x[4] = {0u, 0u, 0u, 0u};

			if (v == 0) {
				uint32_t s[4] = {salt, iv0, iv1, 1u};

				esp_aes_encrypt(rk, nr, s_te, s);
				ej0[0] = s[0];
				ej0[1] = s[1];
				ej0[2] = s[2];
				ej0[3] = s[3];
				x[0] = sad->spi;
				x[1] = seq;
			} else if (v <= nb) {
				const uint32_t b = v - 1u, nbytes = min(16u, E - 16u * b);
				const uint4 ks = keystream(rk, nr, s_te, salt, iv0, iv1, v + 1u);
				uint4 pt = make_uint4(0u, 0u, 0u, 0u);

				if (16u * b < ilen)
					pt = load_bytes(fr + L + 16u * b, min(16u, ilen - 16u * b));
				if (16u * b + 16u > ilen) {
					/* the trailer: pad bytes 1 .. pad, pad, next */
					uint32_t w[4] = {pt.x, pt.y, pt.z, pt.w};

#pragma unroll
					for (uint32_t e = 0; e < 16u; e++) {
						const uint32_t q = 16u * b + e;

						if (q >= ilen && q < E) {
							const uint32_t t = q + 2u < E ? q - ilen + 1u
									 : q + 2u == E ? pad : next;

							w[e >> 2] |= t << (8u * (e & 3u));
						}
					}
					pt = make_uint4(w[0], w[1], w[2], w[3]);
				}
				const uint4 ct = keep_unit(make_uint4(pt.x ^ ks.x, pt.y ^ ks.y, pt.z ^ ks.z,
								      pt.w ^ ks.w), (int32_t)nbytes);

				x[0] = bswap(ct.x);
				x[1] = bswap(ct.y);
				x[2] = bswap(ct.z);
				x[3] = bswap(ct.w);
				o.put_block(p0 + 16u * b, ct, nbytes);
			} else if (v == nb + 1u) {
				x[1] = 64u;
				x[3] = 8u * E;
			}
			ghash_chunk(hpow, l, k, x, y);
			/* blocks up to v - 1 = c G + G - 2 of this chunk are in the ring */
			o.flush(p0 + min(E, 16u * (c * G + G - 1u)));
		}
		if (l == 0) {
			const uint32_t t[4] = {y[0] ^ ej0[0], y[1] ^ ej0[1], y[2] ^ ej0[2], y[3] ^ ej0[3]};

			for (uint32_t k = 0; k < 16u; k++)
				o.put(p0 + E + k, t[k >> 2] >> (24u - 8u * (k & 3u)));
		}
		const uint32_t end = L + tot;

		if (end + l < ((end + 15u) & ~15u))
			o.put(end + l, 0u);
		o.flush((end + 15u) & ~15u);
		return;
	}

	/* ---- inbound ---- */
	const uint32_t C = ilen, ihl = misc, nbc = (C + 15u) >> 4, N = nbc + 2u;
	const uint8_t *esp = fr + L + 4u * ihl, *ct0 = esp + 16;
	const uint32_t seq = a.dst.seq[i];     /* esp_prep parsed it */
	uint32_t iv0, iv1;

	{
		const uint4 iv = load_bytes(esp + 8, 8u);

		iv0 = bswap(iv.x);
		iv1 = bswap(iv.y);
	}
	for (uint32_t c = 0; c * G < N; c++) {
		const uint32_t v = c * G + l, k = min(G, N - c * G);
		uint32_t x[4] = {0u, 0u, 0u, 0u};

		if (v == 0) {
			uint32_t s[4] = {salt, iv0, iv1, 1u};

			esp_aes_encrypt(rk, nr, s_te, s);
			ej0[0] = s[0];
			ej0[1] = s[1];
			ej0[2] = s[2];
			ej0[3] = s[3];
			x[0] = sad->spi;
			x[1] = seq;
		} else if (v <= nbc) {
			const uint32_t b = v - 1u;
			const uint4 ct = load_bytes(ct0 + 16u * b, min(16u, C - 16u * b));

			x[0] = bswap(ct.x);
			x[1] = bswap(ct.y);
			x[2] = bswap(ct.z);
			x[3] = bswap(ct.w);
		} else if (v == nbc + 1u) {
			x[1] = 64u;
			x[3] = 8u * C;
		}
		ghash_chunk(hpow, l, k, x, y);
	}
	uint32_t st = ODPG_ESP_OK;

	{
		const uint4 icv = load_bytes(ct0 + C, 16u);
		const bool same = bswap(icv.x) == (y[0] ^ ej0[0]) && bswap(icv.y) == (y[1] ^ ej0[1]) &&
				  bswap(icv.z) == (y[2] ^ ej0[2]) && bswap(icv.w) == (y[3] ^ ej0[3]);

		/* lane 0 holds E(J0) */
		if (!__shfl((int)same, 0, G))
			st = ODPG_ESP_AUTH;
	}
	/* plaintext block b, its bytes below `upto` of the plaintext */
	auto dec = [&](uint32_t b, uint32_t upto) {
		const uint32_t nbytes = min(16u, upto - 16u * b);
		const uint4 ks = keystream(rk, nr, s_te, salt, iv0, iv1, b + 2u);
		const uint4 ct = load_bytes(ct0 + 16u * b, nbytes);

		return keep_unit(make_uint4(ct.x ^ ks.x, ct.y ^ ks.y, ct.z ^ ks.z, ct.w ^ ks.w),
				 (int32_t)nbytes);
	};
	uint32_t plen = 0;

	if (st == ODPG_ESP_OK) {
		const uint32_t p = byte_of(dec((C - 2u) >> 4, C), (C - 2u) & 15u);
		const uint32_t next = byte_of(dec((C - 1u) >> 4, C), (C - 1u) & 15u);
		uint32_t badpad = p + 2u > C;

		if (!badpad) {
			plen = C - 2u - p;
			for (uint32_t b = (plen >> 4) + l; 16u * b < C - 2u; b += G) {
				const uint4 pt = dec(b, C);

#pragma unroll
				for (uint32_t e = 0; e < 16u; e++) {
					const uint32_t q = 16u * b + e;

					if (q >= plen && q < C - 2u && byte_of(pt, e) != q - plen + 1u)
						badpad = 1;
				}
			}
		}
#pragma unroll
		for (uint32_t m = G / 2u; m; m >>= 1)
			badpad |= __shfl_xor(badpad, m, G);
		if (badpad)
			st = ODPG_ESP_BAD_PAD;
		else if (next != 4u && next != 41u)
			st = ODPG_ESP_BAD_NEXT;
	}
	if (st != ODPG_ESP_OK) {
		if (l == 0) {
			a.dst.status[i] = (uint8_t)st;
			if (fits)
				((uint2 *)a.dst.desc)[i].y = 0;
			atomicSub(&a.dst.total->num_out, 1u);
			atomicMin(&a.dst.total->first_bad, i);
		}
		return;
	}
	if (!fits)
		return;
	const uint32_t nbp = (plen + 15u) >> 4;

	for (uint32_t c = 0; c * G < nbp; c++) {
		const uint32_t b = c * G + l;

		if (b < nbp)
			o.put_block(L + 16u * b, dec(b, plen), min(16u, plen - 16u * b));
		o.flush(L + min(plen, 16u * (c * G + G)));
	}
	const uint32_t end = L + plen;

	if (end + l < ((end + 15u) & ~15u))
		o.put(end + l, 0u);
	o.flush((end + 15u) & ~15u);
	if (l == 0)
		((uint2 *)a.dst.desc)[i].y = end;
}

} /* namespace */

extern "C" int odpg_launch_esp_clear(uint32_t *p, uint32_t words, hipStream_t s)
{
	return rp::clear(p, words, s);
}

extern "C" int odpg_launch_esp(const odpg_esp_args *a, hipStream_t s)
{
	const uint32_t num = a->src.num, ptiles = (num + PWG - 1u) / PWG;
	const bool out = a->dir == ODPG_ESP_OUT;

	if (num) {
		if (out) {
			const Keys keys = {a->skey, num, a->max_sas};
			const rp::Ws ws = {a->order, a->offsets, a->max_sas + 1u, a->key_bits,
					   a->hist, a->dtotal, a->bcount, a->pairs};

			hipLaunchKernelGGL(esp_prep<true>, dim3(ptiles), dim3(PWG), 0, s, *a);
			if (rp::partition(keys, ws, s))
				return -EIO;
			hipLaunchKernelGGL(esp_seq, dim3(ptiles), dim3(PWG), 0, s, *a);
			hipLaunchKernelGGL(esp_advance, dim3((a->max_sas + PWG - 1u) / PWG), dim3(PWG),
					   0, s, *a);
		} else {
			hipLaunchKernelGGL(esp_prep<false>, dim3(ptiles), dim3(PWG), 0, s, *a);
		}
	}
	/* an empty batch: total only */
	hipLaunchKernelGGL(esp_scan, dim3(1), dim3(SCAN_WG), 0, s, *a);
	if (num) {
		hipLaunchKernelGGL(esp_place, dim3(ptiles), dim3(PWG), 0, s, *a);
		if (out)
			hipLaunchKernelGGL(esp_crypt<true>, dim3((num + T - 1u) / T), dim3(WG), 0, s, *a);
		else
			hipLaunchKernelGGL(esp_crypt<false>, dim3((num + T - 1u) / T), dim3(WG), 0, s, *a);
	}
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
