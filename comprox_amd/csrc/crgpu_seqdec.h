/*
 * comprox_amd/csrc/crgpu_seqdec.h — many sequences of dependent comprop, comprox or comprolz blocks DECODED in one launch
 * (crgpu_decode_set, crgpu_decode_sequences_carried*). The text below describes comprop's kernel; what the other two add — the
 * side models, comprolz's matcher tables — stands in front of them.
 *
 * Reference: src/ropmain/cr-coder.c:231-292 (lzdecode: the ppm model survives the block, a stored block does not
 * touch it), src/cr-ppm.c:34-57 (what reset_models() puts back); src/roxmain/cr-coder.c:390-526 and
 * src/rolzmain/cr-coder.c:287-379 for the other two.
 *
 * One sequence is one dependent chain whatever the kernel; the parallel work is other sequences. Unlike the encoder
 * (crgpu_seq.h: lockstep, a host wait per step for the abort point) nothing here has to meet: a block waits for its own
 * predecessor only. So one wave takes a SEQUENCE from the ticket and walks its blocks front to back on the assembly step of
 * crgpu_rop5.h, cr_rop_decode_v5<0, 1, CARRY = 1>; the call is one launch.
 *
 * SLOT: slot s of the set is a whole decoder arena at store + s * stride, laid out as the batched decoder's own
 * (make_layout, crgpu_device.h): directory words, 65 536 node lines, order-1 rows, direct order-3 table, dense area, LZP tables.
 * The models stay where the step keeps them, in the step's format; nothing is converted between blocks or calls.
 *   dense area   65 536 slots of 256 bytes. A node takes a dense slot when it outgrows its line, once per context and generation
 *                (the line then carries the mark until the generation moves on, and only a reset moves it on, which also puts
 *                the counter back to 0): a sequence of any length has no more than one per 16-bit context.
 *   LZP tables   per slot, not per resident workgroup: the step addresses them by 32-bit offsets from the arena it keeps the
 *                models in. They are emptied in front of every block, as matcher_init does.
 *   comprox      no LZP tables; the keep area (L.off_keep, CR_USE_KEEP) that the side models are parked in between calls
 *   comprolz     the keep area, and the matcher's link tables, ring history and ring heads (CR_USE_CAND | CR_USE_HIST |
 *                CR_USE_RHEAD) per slot as well: per-block state that could live per resident workgroup, kept in the slot so
 *                that make_layout serves the set as it serves the batched decoders (a tenth of the slot at 64 KiB)
 *   state words  in the arena's scratch line at CR_SD_OFF_STATE: {fresh, poisoned, context register}. The dense-slot counter is
 *                the step's own word at CRGPU_OFF_SCRATCH + 904; the two generations are the directory words 0 and 3.
 *
 * RESET is lazy: k_seqdec_mark sets `fresh` and clears `poisoned`; the wave that next picks the slot up runs cr_v3_reset
 * (generation bumps, wipe on wrap, order-1 rows = 1) and zeroes the register and the counter.
 *
 * PICK-UP of a slot that is not fresh: generations and register from the slot, and the LDS copies of the dense slots
 * 0 .. min(counter, CR_V5_DLDS) from the arena's dense area, which every store of the step also reaches. They then stay in LDS
 * for all blocks of the sequence: the wave keeps its sequence for the whole launch.
 *
 * FAILURE: a block that fails yields 0xFFFFFFFF, and so does every later block of its slot — their models are unknowable —
 * until the slot is reset; the launch's failed blocks are counted in ticket word 1.
 */
#ifndef CRGPU_SEQDEC_H
#define CRGPU_SEQDEC_H

#include "crgpu_device.h"

#define CR_SD_DENSE_SLOTS 65536u
#define CR_SD_OFF_STATE   (CRGPU_OFF_SCRATCH + 960u)      /* u32 {fresh, poisoned, context register}; the step uses the line up to + 908 */

struct CrSeqDec {
    const uint8_t*  in;
    const u64*      in_off;
    const uint32_t* in_size;
    uint8_t*        out;
    const u64*      out_off;
    const uint32_t* out_cap;
    uint32_t*       out_size;
    const uint32_t* seq_first;  /* device copy: sequence s owns the blocks seq_first[s] .. seq_first[s + 1] - 1 and slot s */
    const uint32_t* order;      /* the sequences that have a block, most coded bytes first */
    uint32_t        nactive;
    uint32_t*       ticket;     /* zeroed before the launch: [0] the next entry of `order`, [1] blocks that failed */
    uint8_t*        store;      /* slot s at store + s * L.stride */
};

/* launchers (crgpu_seqdec.hip) */
void crsd_launch_mark(hipStream_t s, uint8_t* store, u64 stride, const uint32_t* which, uint32_t n);
enum { CR_SD_ROP = 0, CR_SD_ROX = 1, CR_SD_ROLZ = 2 };    /* which: k_seqdec_v5, k_seqdec_rox_v5, k_seqdec_rolz_v5 */
void crsd_launch_decode(hipStream_t s, int which, uint32_t grid, const CrSeqDec& D, const CrArenaLayout& L);
const void* crsd_decode_kernel(int which);               /* for the occupancy query that sizes the grid */
const char* crsd_decode_name(int which);                 /* the kernel's name in the stage log */

#ifdef CRGPU_SEQDEC_TU
#include "crgpu_rop5.h"
#include "crgpu_rox5.h"
#include "crgpu_rolz5.h"

/* slots which[0 .. n) (which == nullptr: slot i) become fresh */
__global__ __launch_bounds__(256) void k_seqdec_mark(uint8_t* store, u64 stride, const uint32_t* which, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t* const state = reinterpret_cast<uint32_t*>(store + (u64)(which ? which[i] : i) * stride + CR_SD_OFF_STATE);
    state[0] = 1u; state[1] = 0u;
}

/* ---- what the three kernels share, as the text of their bodies (in the manner of CR_TICKET_LOOP: k_seqdec_v5 compiles to the
 * code it had when this text stood in it, which a function call does not promise). The kernel has D, L, s_px and lane. ---- */

/* Head of the ticket loop: the next sequence of the launch (most coded bytes first), its blocks b0 .. b1 and its slot, then the
 * PICK-UP (above). fresh_ / resume_ run behind the lazy reset / behind the reload of a slot that continues; a poisoned slot
 * gets neither. Leaves b0, b1, arena, state, poisoned and the carry cy behind. */
#define CR_SD_TAKE_AND_PICK_UP(fresh_, resume_) \
        uint32_t t = 0; \
        if (threadIdx.x == 0) t = atomicAdd(D.ticket, 1u); \
        const uint32_t j = cr_uni(t); \
        if (j >= D.nactive) break; \
        const uint32_t s = cr_uni(D.order[j]); \
        const uint32_t b0 = cr_uni(D.seq_first[s]), b1 = cr_uni(D.seq_first[s + 1u]); \
        uint8_t* const arena = cr_uni_ptr(D.store + (u64)s * L.stride); \
        uint32_t* const state = reinterpret_cast<uint32_t*>(arena + CR_SD_OFF_STATE); \
        uint32_t* const scr = reinterpret_cast<uint32_t*>(arena + CRGPU_OFF_SCRATCH + 896u); \
        bool poisoned = cr_uni(state[1]) != 0u; \
        CrV5Carry cy; \
        cy.ctx = 0u; cy.gen = 0u; cy.g3 = 0u; cy.dslots = L.dense_slots; \
        if (!poisoned) { \
            if (cr_uni(state[0]) != 0u) {                /* reset_models() since the slot's last block */ \
                uint32_t g3; \
                cy.gen = cr_uni(cr_v3_reset(arena, L, g3)); \
                cy.g3 = cr_uni(g3); \
                if (lane == 0) { scr[2] = 0u; state[0] = 0u; state[2] = 0u; } \
                fresh_; \
            } else { \
                const uint32_t* const dir = reinterpret_cast<const uint32_t*>(arena + L.off_dir); \
                cy.gen = cr_uni(dir[0]); cy.g3 = cr_uni(dir[3]); cy.ctx = cr_uni(state[2]); \
                uint32_t nd = cr_uni(scr[2]); \
                if (nd > CR_V5_DLDS) nd = CR_V5_DLDS; \
                const uint32_t* const dense = reinterpret_cast<const uint32_t*>(arena + L.off_dense); \
                for (uint32_t k = 0; k < nd; k++) s_px[68u + k * CRGPU_NODE_WORDS + lane] = dense[k * CRGPU_NODE_WORDS + lane];   /* (the step reads slot k at scratch + 0x110 + 256 k) */ \
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); \
                resume_; \
            } \
        }

/* The sequence's blocks front to back, block b through decode_ (an expression that yields its size or 0xFFFFFFFF). A block
 * that fails poisons the slot; it and every block behind it report 0xFFFFFFFF and are counted. */
#define CR_SD_WALK(decode_) \
        for (uint32_t b = b0; b < b1; b++) { \
            uint32_t r = 0xFFFFFFFFu; \
            if (!poisoned) { \
                r = decode_; \
                if (r == 0xFFFFFFFFu) { poisoned = true; if (lane == 0) state[1] = 1u; } \
            } \
            if (lane == 0) { \
                D.out_size[b] = r; \
                if (r == 0xFFFFFFFFu) atomicAdd(D.ticket + 1, 1u); \
            } \
            cr_wave_sync(); \
        }

/* One wave per workgroup, as many workgroups as are resident (or sequences). The LDS is k_rop_decode_v5's: 272 scratch bytes,
 * CR_V5_DLDS dense nodes, the spare slot. */
__global__ __launch_bounds__(CRGPU_WAVE) void k_seqdec_v5(CrSeqDec D, CrArenaLayout L) {
    __shared__ __attribute__((aligned(256))) uint32_t s_px[CR_V5_LDS_BYTES / 4u];
    const uint32_t s_px_at = (uint32_t)reinterpret_cast<uintptr_t>(&s_px[0]);
    __builtin_amdgcn_s_setprio(3);                      /* a dependent chain: its instructions go first when another stream's kernels share the SIMD */
    const uint32_t lane = cr_lane();
    for (;;) {
        CR_SD_TAKE_AND_PICK_UP((void)0, (void)0)
        CR_SD_WALK((cr_rop_decode_v5<0, 1, 1>(D.in + D.in_off[b], D.in_size[b], D.out + D.out_off[b], D.out_cap[b], arena, L, s_px_at, nullptr, &cy)))
        if (!poisoned && lane == 0) state[2] = cy.ctx;
        cr_wave_sync();
    }
}

/* ---- comprox and comprolz (crgpu_rox5.h, crgpu_rolz5.h with CARRY): beside the ppm model the reference carries eight
 * (src/roxmain/cr-coder.c:55-60,88-114) / two (src/rolzmain/cr-coder.c:52-60,78-97) side models. They live in LDS (CrRoxShared)
 * for the whole sequence: reset at a fresh pick-up, loaded from the slot's keep area (L.off_keep, cr_side_unpark) at one that
 * continues, parked there once when the wave leaves the sequence unpoisoned, next to the register's store. A stored block
 * touches neither them nor the register. Everything else is per block, inside the wrappers. ---- */

/* the wave leaves its sequence: register and side models go back to the slot unless a block has poisoned it */
CR_DEV void cr_sd_side_leave(uint8_t* arena, const CrArenaLayout& L, const CrRoxShared& sh, uint32_t ctx, bool poisoned) {
    if (!poisoned) {
        if (cr_lane() == 0) reinterpret_cast<uint32_t*>(arena + CR_SD_OFF_STATE)[2] = ctx;
        cr_side_park(sh, arena + L.off_keep);
    }
    cr_wave_sync();
}

__global__ __launch_bounds__(CRGPU_WAVE) void k_seqdec_rox_v5(CrSeqDec D, CrArenaLayout L) {
    __shared__ CrRoxShared sh;
    __shared__ __attribute__((aligned(256))) uint32_t s_px[CR_V5_LDS_BYTES / 4u];
    const uint32_t s_px_at = (uint32_t)reinterpret_cast<uintptr_t>(&s_px[0]);
    __builtin_amdgcn_s_setprio(3);
    const uint32_t lane = cr_lane();
    for (;;) {
        CR_SD_TAKE_AND_PICK_UP(cr_side_reset(sh), cr_side_unpark(sh, arena + L.off_keep))
        CR_SD_WALK((cr_rox_decode_v5<1>(D.in + D.in_off[b], D.in_size[b], D.out + D.out_off[b], D.out_cap[b], arena, L, sh, s_px_at, &cy)))
        cr_sd_side_leave(arena, L, sh, cy.ctx, poisoned);
    }
}

/* comprolz's matcher is per block (matcher_init inside every lzdecode, cr-coder.c:321): its link tables, ring heads and ring
 * history are the slot's own regions (CR_USE_CAND | CR_USE_HIST | CR_USE_RHEAD), refilled by the wrapper in front of every
 * block; the row heads are in LDS. */
__global__ __launch_bounds__(CRGPU_WAVE) void k_seqdec_rolz_v5(CrSeqDec D, CrArenaLayout L) {
    __shared__ CrRoxShared sh;
    __shared__ uint32_t s_rows[256];
    __shared__ __attribute__((aligned(256))) uint32_t s_px[CR_V5_LDS_BYTES / 4u];
    const uint32_t s_px_at = (uint32_t)reinterpret_cast<uintptr_t>(&s_px[0]);
    __builtin_amdgcn_s_setprio(3);
    const uint32_t lane = cr_lane();
    for (;;) {
        CR_SD_TAKE_AND_PICK_UP(cr_rolz_side_reset(sh), cr_side_unpark(sh, arena + L.off_keep))
        CrRolzTables T;
        T.ring_prev = reinterpret_cast<uint32_t*>(arena + L.off_cand);            /* u32[3][max_block]: two of the three */
        T.row_prev = T.ring_prev + L.max_block;
        T.rank = nullptr; T.len = nullptr; T.ring16 = nullptr; T.raw16 = nullptr; T.row16 = nullptr;
        T.ring_head = reinterpret_cast<uint32_t*>(arena + L.off_rolz_head);
        uint32_t* const hist = L.off_hist ? reinterpret_cast<uint32_t*>(arena + L.off_hist) : nullptr;
        CR_SD_WALK((cr_rolz_decode_v5<1>(D.in + D.in_off[b], D.in_size[b], D.out + D.out_off[b], D.out_cap[b], T, s_rows, arena, L, sh, hist, s_px_at, nullptr, &cy)))
        cr_sd_side_leave(arena, L, sh, cy.ctx, poisoned);
    }
}

#undef CR_SD_TAKE_AND_PICK_UP
#undef CR_SD_WALK

#endif /* CRGPU_SEQDEC_TU */
#endif
