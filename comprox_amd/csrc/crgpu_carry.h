/*
 * comprox_amd/csrc/crgpu_carry.h — comprop's chain encoder with models that outlive the block (crgpu_models,
 * crgpu_encode_blocks_carried*).
 *
 * The reference's ppm_model_t (src/cr-ppm.h:36-41) survives from one lzencode to the next until reset_models(); the kernels of
 * crgpu_rop2.h start every chain from the empty model. Here the model lives in a STORE in device memory, indexed by the
 * reference's own keys — no hashing, and no two chains of a block ever touch the same cell:
 *   order-1 rows    u8[256][256]                                                          65 536 bytes
 *   order-2 records [65 536] x 272 bytes: the 256 byte counts, then one word               17 825 792
 *                   count(256) | count(257) << 8 | sum of the byte counts << 16
 *   order-3 cells   u16[1 << 22]: predicted byte | confidence << 8, one per 22-bit key       8 388 608
 *   context         the 32-bit register (cr-ppm.c:60-64), in a 256-byte tail                       256
 *                                                                                    = 26 280 192 bytes
 * A chain's state is loaded where the chain starts and stored where it ends: one record per chain and direction, nothing per
 * event. The event sorts (k_rop_links*) and the range coder (k_rop_rc) need no model and are the kernels of crgpu_rop2.h /
 * crgpu_links2.h; a call runs them and the kernels below block after block.
 *
 *   k_ropc_fill     the store in the ppm_model_init state (cr-ppm.c:34-48)
 *   k_ropc_events   k_rop_events with the store's context register in front of the first token and behind the last
 *   k_ropc_o3       one lane per order-3 chain, ANY number of workgroups: chains of one block are independent, their cells disjoint
 *   k_ropc_o2       one lane per order-2 chain, the node in the lane's slice of LDS, built from the chain's record and written
 *                   back; chains handed out by one counter in device memory, so the block's chains spread over the whole chip
 *   k_ropc_o1       k_rop_o1 with every row started from and written back to the store
 *   k_ropc_abort    the token at which lzencode gave the block up (cr-coder.c:204-206): the models stay as they stood THERE, so
 *                   the host restores its copy of the store and runs the chain kernels again over the events up to that token
 *
 * The kernels are a translation unit of their own (crgpu_carry.hip defines CRGPU_CARRY_TU and holds their launchers): the code
 * of the kernels in crgpu.hip does not move by a byte when these change, and the other way round.
 */
#ifndef CRGPU_CARRY_H
#define CRGPU_CARRY_H

#include "crgpu_device.h"

#define CR_M_O2_REC   272u
#define CR_M_OFF_O1   0ull
#define CR_M_OFF_O2   65536ull
#define CR_M_OFF_O3   (CR_M_OFF_O2 + 65536ull * CR_M_O2_REC)
#define CR_M_OFF_CTX  (CR_M_OFF_O3 + (1ull << 22) * 2ull)
#define CR_M_BYTES    (CR_M_OFF_CTX + 256ull)
/* words of CrBatch::ticket and of the event scratch's counter line the kernels here use */
#define CR_TK_CARRY_CHAIN 20
#define CR_CTR_END_CTX    9u          /* ctr[9]: the context register behind the block's last token */
#define CR_O2C_THREADS    64u

/* launchers (crgpu_carry.hip); B1 describes ONE block: every per-block pointer of the batch moved on to it, nblocks = 1 */
void crc_launch_fill(hipStream_t s, uint32_t grid, uint8_t* M);
void crc_launch_events(hipStream_t s, const CrBatch& B1, const CrArenaLayout& L, uint8_t* M);
void crc_launch_o3(hipStream_t s, uint32_t grid, const CrBatch& B1, uint8_t* M);
void crc_launch_o2(hipStream_t s, uint32_t grid, const CrBatch& B1, uint8_t* M);
void crc_launch_o1(hipStream_t s, const CrBatch& B1, uint8_t* M);
void crc_launch_abort(hipStream_t s, const CrBatch& B1, uint8_t* M);

/* CRGPU_CARRY_FUNCS: the chain walkers below without the kernels, for a translation unit with kernels of its own (crgpu_seq.h) */
#if defined(CRGPU_CARRY_TU) || defined(CRGPU_CARRY_FUNCS)
#include "crgpu_rop2.h"

#ifdef CRGPU_CARRY_TU
/* ppm_model_init: every order-1 count 1, no order-2 byte seen (flag counts 1 / 1), order-3 cells and the register 0 */
__global__ __launch_bounds__(256) void k_ropc_fill(uint8_t* M) {
    const u64 words = CR_M_BYTES / 16u;
    for (u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (u64)gridDim.x * blockDim.x) {
        const u64 o = w * 16u;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (o < CR_M_OFF_O2) v = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
        else if (o < CR_M_OFF_O3 && (o - CR_M_OFF_O2) % CR_M_O2_REC == 256u) v.x = 0x0101u;
        reinterpret_cast<uint4*>(M)[w] = v;
    }
}
#endif

/* ------------------------------------------------------------------ order 3 */

/* cr_rop_o3_chain with the table entry taken from and returned to the store. The chain's key comes from its first event's
 * context (order-3 slot -> order-2 slot -> event): three dependent loads, once per chain. A carried chain may predict a byte
 * at its first event already, so every prediction is stored, 0 included (the sorts cleared cpred in passing; storing a 0 over
 * it is only a request more). LOG (crgpu_seq.h): the chain's start state {key, old cell} goes to *log before the walk */
template <bool LOG = false>
CR_DEV void cr_ropc_o3_chain(CrEvViews& V, uint16_t* o3, uint32_t s, uint2* log = nullptr) {
    uint32_t n_sym = V.csym3[s], n_slot = V.cslot3[s];
    const uint32_t key = cr_o3_key(V.ev_ctx[V.list2[n_slot]]);
    const uint32_t cell = o3[key];
    if constexpr (LOG) *log = make_uint2(key, cell);
    uint32_t pred = cell & 0xffu, conf = cell >> 8;
    for (;;) {
        const uint32_t sy = n_sym, slot = n_slot;
        const bool last = (sy & 0x8000u) != 0u;
        s++;
        if (!last) { n_sym = V.csym3[s]; n_slot = V.cslot3[s]; }
        const uint32_t sym = sy & 0x1ffu;
        V.cpred[slot] = (uint8_t)pred;
        if (sym == pred) {
            conf += conf < 15u ? 1u : 0u;
        } else {
            uint32_t c = (uint32_t)(conf > 1u) + (uint32_t)(conf > 2u) + (uint32_t)(conf > 4u) + (uint32_t)(conf > 8u);
            if (c == 0u) { pred = sym & 0xffu; c = 1u; }                   /* (comprop's symbols are bytes: cr-ppm.c:79 stores a u8) */
            conf = c;
        }
        if (last) break;
    }
    o3[key] = (uint16_t)(pred | (conf << 8));
}

#ifdef CRGPU_CARRY_TU
__global__ __launch_bounds__(256) void k_ropc_o3(CrBatch B, uint8_t* M) {
    CrEvViews V = cr_ev_views(B.ev, B.ev_cap);
    const uint32_t nev = V.ctr[0];
    const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x, gn = gridDim.x * blockDim.x;
    /* (the triples start out as CR_TRIP_FRESH: cr_rop_o2_event stores only the ones that differ — whatever the node held) */
    for (uint32_t i = gt * 2u; i < nev; i += gn * 2u) { const u64 f = CR_TRIP_FRESH; *reinterpret_cast<ulonglong2*>(V.trip + i) = make_ulonglong2(f, f); }
    const uint32_t nc = nev ? V.ctr[2] : 0u;
    uint16_t* const o3 = reinterpret_cast<uint16_t*>(M + CR_M_OFF_O3);
    for (uint32_t c = gt; c < nc; c += gn) cr_ropc_o3_chain(V, o3, V.starts3[c]);
}
#endif

/* ------------------------------------------------------------------ order 2 */

/* the lane's node from a record: the flag word first — a context never seen holds no byte, its counts are not fetched —, else
 * the 256 counts in sixteen 16-byte loads, the group sums and the "has a count" set worked out on the way in (as cr_ln_halve
 * does on its way through) */
CR_DEV void cr_ln_load(CrLaneNode& nd, const uint8_t* rec) {
    const uint32_t fl = *reinterpret_cast<const uint32_t*>(rec + 256u);
    nd.fh = fl & 0xffu; nd.fe = (fl >> 8) & 0xffu; nd.bytes = fl >> 16;
    if (nd.bytes == 0u) {
        for (uint32_t q = 0; q < 20u; q++) reinterpret_cast<uint4*>(nd.cnt)[q] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    uint4 v[16];
#pragma unroll
    for (uint32_t q = 0; q < 16u; q++) v[q] = reinterpret_cast<const uint4*>(rec)[q];
#pragma unroll
    for (uint32_t gi = 0; gi < 8u; gi++) {
        uint32_t gs = 0, bits = 0;
#pragma unroll
        for (uint32_t h = 0; h < 2u; h++) {
            const uint4 x = v[gi * 2u + h];
            reinterpret_cast<uint4*>(nd.cnt + gi * 32u)[h] = x;
            gs += cr_ln_sum4(x.x) + cr_ln_sum4(x.y) + cr_ln_sum4(x.z) + cr_ln_sum4(x.w);
            bits |= (cr_nz4(x.x) | (cr_nz4(x.y) << 4) | (cr_nz4(x.z) << 8) | (cr_nz4(x.w) << 12)) << (h * 16u);
        }
        reinterpret_cast<uint32_t*>(nd.cnt + CR_LN_G)[gi] = gs;
        reinterpret_cast<uint32_t*>(nd.cnt + CR_LN_NZ)[gi] = bits;
    }
}
/* ... and back. A node that still holds no byte was loaded from a record of zeros: only the flag word has moved */
CR_DEV void cr_ln_save(const CrLaneNode& nd, uint8_t* rec) {
    if (nd.bytes) {
#pragma unroll
        for (uint32_t q = 0; q < 16u; q++) reinterpret_cast<uint4*>(rec)[q] = reinterpret_cast<const uint4*>(nd.cnt)[q];
    }
    *reinterpret_cast<uint32_t*>(rec + 256u) = nd.fh | (nd.fe << 8) | (nd.bytes << 16);
}

/* cr_rop_o2_all with the chain's record around it. The record's address comes from the first event's context, fetched with
 * the chain's first operands; cr_rop_o2_event's shortcuts (an empty node stores no exclusion set, a triple equal to
 * CR_TRIP_FRESH is not stored) test the node itself, and the node is what the store says. LOG (crgpu_seq.h): chain h writes
 * its start state to the 280-byte record h of `log` — the record's 256 counts if it holds any, its flag word at 256, the
 * context at 260 — in 8-byte pieces (280 is no multiple of 16) */
template <bool LOG = false>
CR_DEV void cr_ropc_o2_all(CrEvViews& V, uint8_t* lane_node, uint8_t* o2, uint32_t nchains, uint32_t* next_chain /* device memory */, uint8_t* log = nullptr) {
    CrLaneNode nd;
    nd.cnt = lane_node; nd.bytes = 0; nd.fh = 1; nd.fe = 1;
    uint32_t at = 0, end = 0;
    uint32_t n_i = 0, n_sp = 0;
    uint8_t* rec = nullptr;
    for (;;) {
        if (at == end) {
            if (rec) { cr_ln_save(nd, rec); rec = nullptr; }
            const uint32_t h = atomicAdd(next_chain, 1u);
            if (h >= nchains) break;
            const u64 ch = V.chains2[h];
            at = (uint32_t)ch; end = (uint32_t)(ch >> 32);
            n_i = V.list2[at]; n_sp = (uint32_t)V.csym2[at] | ((uint32_t)V.cpred[at] << 16);
            rec = o2 + (u64)(V.ev_ctx[n_i] & 0xffffu) * CR_M_O2_REC;
            if constexpr (LOG) {
                uint2* const lr = reinterpret_cast<uint2*>(log + (u64)h * 280u);
                const uint32_t fl = *reinterpret_cast<const uint32_t*>(rec + 256u);
                lr[32] = make_uint2(fl, V.ev_ctx[n_i] & 0xffffu);
                if (fl >> 16) {
#pragma unroll
                    for (uint32_t q = 0; q < 32u; q++) lr[q] = reinterpret_cast<const uint2*>(rec)[q];
                }
            }
            cr_ln_load(nd, rec);
        }
        const uint32_t i = n_i, sp = n_sp;
        at++;
        if (at < end) { n_i = V.list2[at]; n_sp = (uint32_t)V.csym2[at] | ((uint32_t)V.cpred[at] << 16); }
        cr_rop_o2_event(V, nd, i, sp & 0x1ffu, sp >> 16);
    }
}

/* the abort point of a block of n bytes that ended stored: the event-by-event coder of cr_code_events run until the token
 * loop's test fires (`header` = the bytes the block format puts in front of the stream), its bytes into scratch (escB, dead
 * since the order-1 pass; a step can release a run of held-back bytes, the region is 8 bytes per event slot). Returns the
 * number of events up to and including that token */
CR_DEV uint32_t cr_ropc_abort_cut(const CrEvViews& V, uint32_t n, uint32_t nev, uint32_t header) {
    CrSink out; out.dst = reinterpret_cast<uint8_t*>(V.escB); out.n = 0;
    CrRc rc; cr_rc_init(rc);
    CrEvWindow w;
    cr_evwin_fill(w, V, 0, nev);
    for (uint32_t i = 0; i < nev; i++) {
        if (i - w.base >= CRGPU_WAVE) cr_evwin_fill(w, V, i, nev);
        const uint32_t l = i - w.base;
        const u64 t = cr_lane_get64(w.trip, l);
        cr_rc_pin(rc); out.n = cr_uni(out.n);
        cr_rc_encode(rc, (uint32_t)t & 0xfffffu, (uint32_t)(t >> 40) & 0x3ffu, (uint32_t)(t >> 20) & 0xfffffu, out);
        if (((uint32_t)(t >> 50) & 3u) == CR_T_ESC) {
            const u64 t2 = cr_lane_get64(w.trip2, l);
            cr_rc_pin(rc); out.n = cr_uni(out.n);
            cr_rc_encode(rc, (uint32_t)t2 & 0xfffffu, (uint32_t)(t2 >> 40) & 0xfffu, (uint32_t)(t2 >> 20) & 0xfffffu, out);
        }
        if ((cr_lane_get(w.sym, l) & CR_EV_LAST) && header + out.n >= n) return i + 1u;
    }
    return nev;
}

#ifdef CRGPU_CARRY_TU
__global__ __launch_bounds__(CR_O2C_THREADS) void k_ropc_o2(CrBatch B, uint8_t* M) {
    __shared__ __attribute__((aligned(16))) uint8_t s_nodes[CR_O2C_THREADS * CR_LN_STRIDE];
    CrEvViews V = cr_ev_views(B.ev, B.ev_cap);
    const uint32_t nev = V.ctr[0];
    const uint32_t nc = nev ? V.ctr[1] : 0u;
    cr_ropc_o2_all(V, s_nodes + threadIdx.x * CR_LN_STRIDE, M + CR_M_OFF_O2, nc, B.ticket + CR_TK_CARRY_CHAIN);
}

/* ------------------------------------------------------------------ events, order 1 */

__global__ __launch_bounds__(CRGPU_WAVE) void k_ropc_events(CrBatch B, CrArenaLayout L, uint8_t* M) {
    __shared__ CrShared sh;
    const uint32_t n = B.in_size[0];
    CrEvViews V = cr_ev_views(B.ev, B.ev_cap);
    uint32_t* const ctx = reinterpret_cast<uint32_t*>(M + CR_M_OFF_CTX);
    if (n <= L.max_block) {
        cr_rop_emit_events<true>(B.in + B.in_off[0], n, B.lens, V, sh, ctx);
        if (threadIdx.x == 0) V.ctr[CR_CTR_END_CTX] = *ctx;
    } else if (threadIdx.x == 0) { V.ctr[0] = 0; V.ctr[1] = 0; V.ctr[2] = 0; V.ctr[3] = 0x200u; }
}

__global__ __launch_bounds__(CR_O1_THREADS) void k_ropc_o1(CrBatch B, uint8_t* M) {
    __shared__ CrSortShared sh;
    static_assert(sizeof(sh.buf) >= CR_SORT_WAVES * CR_O1_LDS_PER_WAVE * 4u, "the order-1 rows' LDS lies over the sort tile");
    uint32_t* const s_masks = reinterpret_cast<uint32_t*>(sh.buf);
    CrEvViews V = cr_ev_views(B.ev, B.ev_cap);
    const uint32_t nev = (V.ctr[3] & 0x300u) ? 0u : V.ctr[0];
    if (nev) cr_rop_o1_all(sh, V, s_masks, nev, B.o2_tickets, nullptr, M + CR_M_OFF_O1);
}

/* ------------------------------------------------------------------ the abort point */

/* One wave, behind k_rop_rc, for a block that ended stored although it has events: cr_ropc_abort_cut finds the token at which
 * the token loop's test fires (cr-coder.c:204-206). The block's event count
 * becomes the events up to and including that token, and the store's register the context in front of the NEXT token — the
 * token's own updates applied —, which is the next event's context or, behind the last token, what k_ropc_events left. The
 * host has put its copy of the store back before this runs. */
__global__ __launch_bounds__(CRGPU_WAVE) void k_ropc_abort(CrBatch B, uint8_t* M) {
    CrEvViews V = cr_ev_views(B.ev, B.ev_cap);
    const uint32_t n = B.in_size[0];
    const uint32_t nev = cr_uni(V.ctr[0]);
    if ((cr_uni(V.ctr[3]) & 0x300u) || nev == 0u) return;
    const uint32_t keep = cr_ropc_abort_cut(V, n, nev, CR_ROP_HEADER);
    if (cr_lane() == 0) {
        *reinterpret_cast<uint32_t*>(M + CR_M_OFF_CTX) = keep < nev ? V.ev_ctx[keep] : V.ctr[CR_CTR_END_CTX];
        V.ctr[0] = keep;
    }
}

#endif /* CRGPU_CARRY_TU: the kernels */
#endif /* CRGPU_CARRY_TU || CRGPU_CARRY_FUNCS */
#endif
