/*
 * comprox_amd/csrc/crgpu_seqdec.h — many sequences of dependent comprop blocks DECODED in one launch (crgpu_decode_set,
 * crgpu_decode_sequences_carried*).
 *
 * Reference: src/ropmain/cr-coder.c:231-292 (lzdecode: the ppm model survives the block, a stored block does not
 * touch it), src/cr-ppm.c:34-57 (what reset_models() puts back).
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
void crsd_launch_decode(hipStream_t s, uint32_t grid, const CrSeqDec& D, const CrArenaLayout& L);
const void* crsd_decode_kernel(void);                    /* for the occupancy query that sizes the grid */

#ifdef CRGPU_SEQDEC_TU
#include "crgpu_rop5.h"

/* slots which[0 .. n) (which == nullptr: slot i) become fresh */
__global__ __launch_bounds__(256) void k_seqdec_mark(uint8_t* store, u64 stride, const uint32_t* which, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t* const state = reinterpret_cast<uint32_t*>(store + (u64)(which ? which[i] : i) * stride + CR_SD_OFF_STATE);
    state[0] = 1u; state[1] = 0u;
}

/* One wave per workgroup, as many workgroups as are resident (or sequences). The LDS is k_rop_decode_v5's: 272 scratch bytes,
 * CR_V5_DLDS dense nodes, the spare slot. */
__global__ __launch_bounds__(CRGPU_WAVE) void k_seqdec_v5(CrSeqDec D, CrArenaLayout L) {
    __shared__ __attribute__((aligned(256))) uint32_t s_px[CR_V5_LDS_BYTES / 4u];
    const uint32_t s_px_at = (uint32_t)reinterpret_cast<uintptr_t>(&s_px[0]);
    __builtin_amdgcn_s_setprio(3);                      /* a dependent chain: its instructions go first when another stream's kernels share the SIMD */
    const uint32_t lane = cr_lane();
    for (;;) {
        uint32_t t = 0;
        if (threadIdx.x == 0) t = atomicAdd(D.ticket, 1u);
        const uint32_t j = cr_uni(t);
        if (j >= D.nactive) break;
        const uint32_t s = cr_uni(D.order[j]);
        const uint32_t b0 = cr_uni(D.seq_first[s]), b1 = cr_uni(D.seq_first[s + 1u]);
        uint8_t* const arena = cr_uni_ptr(D.store + (u64)s * L.stride);
        uint32_t* const state = reinterpret_cast<uint32_t*>(arena + CR_SD_OFF_STATE);
        uint32_t* const scr = reinterpret_cast<uint32_t*>(arena + CRGPU_OFF_SCRATCH + 896u);
        bool poisoned = cr_uni(state[1]) != 0u;
        CrV5Carry cy;
        cy.ctx = 0u; cy.gen = 0u; cy.g3 = 0u; cy.dslots = L.dense_slots;
        if (!poisoned) {
            if (cr_uni(state[0]) != 0u) {                /* reset_models() since the slot's last block */
                uint32_t g3;
                cy.gen = cr_uni(cr_v3_reset(arena, L, g3));
                cy.g3 = cr_uni(g3);
                if (lane == 0) { scr[2] = 0u; state[0] = 0u; state[2] = 0u; }
            } else {
                const uint32_t* const dir = reinterpret_cast<const uint32_t*>(arena + L.off_dir);
                cy.gen = cr_uni(dir[0]); cy.g3 = cr_uni(dir[3]); cy.ctx = cr_uni(state[2]);
                uint32_t nd = cr_uni(scr[2]);
                if (nd > CR_V5_DLDS) nd = CR_V5_DLDS;
                const uint32_t* const dense = reinterpret_cast<const uint32_t*>(arena + L.off_dense);
                for (uint32_t k = 0; k < nd; k++) s_px[68u + k * CRGPU_NODE_WORDS + lane] = dense[k * CRGPU_NODE_WORDS + lane];   /* (the step reads slot k at scratch + 0x110 + 256 k) */
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            }
        }
        for (uint32_t b = b0; b < b1; b++) {
            uint32_t r = 0xFFFFFFFFu;
            if (!poisoned) {
                r = cr_rop_decode_v5<0, 1, 1>(D.in + D.in_off[b], D.in_size[b], D.out + D.out_off[b], D.out_cap[b], arena, L, s_px_at, nullptr, &cy);
                if (r == 0xFFFFFFFFu) { poisoned = true; if (lane == 0) state[1] = 1u; }
            }
            if (lane == 0) {
                D.out_size[b] = r;
                if (r == 0xFFFFFFFFu) atomicAdd(D.ticket + 1, 1u);
            }
            cr_wave_sync();
        }
        if (!poisoned && lane == 0) state[2] = cy.ctx;
        cr_wave_sync();
    }
}

#endif /* CRGPU_SEQDEC_TU */
#endif
