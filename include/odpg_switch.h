/* SPDX-License-Identifier: BSD-3-Clause
 *
 * odpg_switch.h — L2 learning-switch forwarding of a device-resident batch.
 *
 * The batch form of the reference's example/switch: every frame teaches the
 * MAC table its source address and ingress port, looks its destination up and
 * is sent to one port or flooded to all others. The reference's workers race
 * on the table; this batch form is defined as the sequential run of
 * forward_packets (odp_switch.c:563-607) over the batch in index order, with
 * one tick for the whole batch. It is deterministic: every output and the
 * table are byte-identical from run to run. Kept from the reference: the
 * direct-mapped table, slot = odp_hash_crc32c(mac, 6, 0) & 0xFFFF (:173-180),
 * the entry {mac[6], port, tick} in one 64-bit word (:53-61; on little-endian
 * bytes 0-5 the MAC, byte 6 the port, byte 7 the tick), a write replacing
 * whatever the slot held (mac_table_update :231-247), and the aging test of
 * mac_table_get (:204-222): an entry hits iff its six MAC bytes are equal and
 * diff_ticks(cur_tick, entry.tick) <= ODPG_SWITCH_AGING_TIME, diff_ticks
 * (:185-192) being t2 - t1 if t1 < t2, (uint8_t)(255 + t2 - t1) if t1 > t2,
 * else 0, with t1 the entry's tick and t2 cur_tick. The reference declares
 * MAC_TBL_SIZE as UINT16_MAX, so slot 0xFFFF lies one past its array; the
 * device table has 65536 entries and slot 0xFFFF is an ordinary slot.
 *
 * Per-packet rules. fr is the frame, n its length, dst = fr[0, 6),
 * src = fr[6, 12), port_in the packet's ingress port.
 *  1. n < 14: status DROP_FRAME. This library's reading of "no Ethernet
 *     header" (:577-581).
 *  2. port_in >= num_ports: status DROP_PORT.
 *  3. check_frame (:528-547) says invalid (src is ff:ff:ff:ff:ff:ff, src is
 *     all-zero or dst is all-zero): status DROP_FRAME.
 *  4. A dropped packet neither learns nor forwards: it writes no slot and is
 *     in no list.
 *  5. Every other packet first writes {src, port_in, cur_tick} to src's slot
 *     (:594).
 *  6. It then reads dst's slot as left by all packets with index <= i, its own
 *     write included: a frame whose source equals its destination hits
 *     itself. Where no packet up to i wrote that slot, it reads the table as
 *     it stood before the call, with the aging test. A slot written during
 *     the call carries cur_tick, so it hits iff its MAC equals dst.
 *  7. A broadcast dst or a miss gives FLOOD (:597-600), a hit gives UNICAST
 *     with the entry's port (:602-605), with no test against port_in.
 *  8. out[i] = kind << 8 | port: port is the entry's port for UNICAST and 0
 *     otherwise.
 *     A preloaded entry whose port is >= num_ports still gives UNICAST
 *     with that port; the packet is then in no list.
 *  9. After the call each written slot holds its last writer's entry; other
 *     slots are unchanged.
 *
 * Per-port lists. Port p's list is lists[p * list_stride + k], k < count[p]:
 * the indices that are UNICAST to p, or FLOOD with port_in != p, strictly
 * ascending: the order of the reference's per-port TX buffer. port_offsets
 * [2 p] = 0 and port_offsets[2 p + 1] = count[p], so port p goes straight
 * into odpg_gather(g, src, lists + p * list_stride, port_offsets + 2 * p, 0,
 * 1, dst): the one-bucket convention odpg_reass uses for `held`. (One
 * concatenated list would not do: odpg_gather clamps list ends to src->num
 * and flooding makes more entries than packets.) List words at and beyond
 * count[p] are not written. A frame that is flooded appears under several
 * ports: the replication broadcast_packet (:491-519) does with
 * odp_packet_copy.
 *
 * A frame is read in one 16-byte unit at its start, inside
 * [offset, offset + align16(len)), and only if n >= 14. Not covered: the
 * reference's per-port statistics, VLANs, a tick source (the caller passes
 * cur_tick as the reference's workers read their global tick).
 */
#ifndef ODPG_SWITCH_H_
#define ODPG_SWITCH_H_

#include "odpg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kind of out[i] */
#define ODPG_SWITCH_UNICAST    0u
#define ODPG_SWITCH_FLOOD      1u
#define ODPG_SWITCH_DROP_FRAME 2u
#define ODPG_SWITCH_DROP_PORT  3u
#define ODPG_SWITCH_KIND(w) ((uint32_t)(w) >> 8)
#define ODPG_SWITCH_PORT(w) ((uint32_t)(w) & 0xFFu)

#define ODPG_SWITCH_MAX_PORTS  32u      /* ODPG_FWD_MAX_PORTS; a 32-bit port mask */
#define ODPG_SWITCH_TABLE_SIZE 65536u   /* entries of the MAC table */
#define ODPG_SWITCH_AGING_TIME 5u       /* ticks (AGING_TIME, odp_switch.c:46) */

/* Packets one workgroup of the resolve and list kernels handles (switch.hip).
 * Informative: batches are of any size; sizes around multiples of it are where
 * the kernels change shape. */
#define ODPG_SWITCH_TILE 256u

typedef struct odpg_switch_s odpg_switch_t;

typedef struct odpg_switch_src_s {
	const uint8_t     *frames;       /* device */
	const odpg_desc_t *desc;         /* device, or NULL: fixed stride, len = stride */
	uint32_t           stride;       /* multiple of 16 when desc == NULL */
	uint32_t           num;
	const uint8_t     *port_in;      /* device, one per packet, or NULL */
	uint8_t            uniform_port; /* every packet's ingress port when port_in == NULL */
	uint8_t            reserved[7];
} odpg_switch_src_t;

typedef struct odpg_switch_total_s {  /* device, written by every call */
	uint32_t unicast;
	uint32_t flooded;
	uint32_t dropped;   /* DROP_FRAME and DROP_PORT */
	uint32_t entries;   /* list entries over all ports */
} odpg_switch_total_t;

typedef struct odpg_switch_dst_s {
	uint32_t            *out;          /* device, src->num words */
	uint32_t            *lists;        /* device, num_ports x list_stride words */
	uint32_t             list_stride;  /* >= src->num */
	uint32_t             reserved;
	uint32_t            *port_offsets; /* device, 2 x num_ports words */
	odpg_switch_total_t *total;        /* device */
} odpg_switch_dst_t;

/* Plan: the MAC table (ODPG_SWITCH_TABLE_SIZE 64-bit entries, zeroed here) and
 * the device workspace for batches of up to max_pkts frames, at most 2^24, on
 * num_ports ports, 2 to ODPG_SWITCH_MAX_PORTS. -EINVAL outside those. Holds a
 * context reference like counters do (odpg.h "object lifetimes"). */
int  odpg_switch_create(odpg_ctx_t *ctx, uint32_t num_ports, uint32_t max_pkts,
			odpg_switch_t **plan);
void odpg_switch_destroy(odpg_switch_t *plan);

/* The device address of the table. Between batches a caller saves, preloads
 * or clears it with odpg_memcpy_d2h / odpg_memcpy_h2d / odpg_memset_dev, which
 * are ordered with the calls on the context stream. NULL for a null plan. */
uint64_t *odpg_switch_table(odpg_switch_t *plan);

/* Asynchronous on the context stream; allocates nothing; no host sync.
 * num == 0 writes *total and port_offsets only. -EINVAL, with nothing
 * launched, for a null plan, src, dst, dst->out, dst->lists,
 * dst->port_offsets or dst->total (or src->frames with src->num != 0), a
 * frames pointer that is not 16-byte aligned, a fixed stride that is zero or
 * no multiple of 16, src->num > max_pkts and list_stride < src->num. One call
 * at a time per plan. */
int  odpg_switch(odpg_switch_t *plan, const odpg_switch_src_t *src, uint8_t cur_tick,
		 const odpg_switch_dst_t *dst);

#ifdef __cplusplus
}
#endif

#endif /* ODPG_SWITCH_H_ */
