/*
 * comprox_amd/csrc/crgpu_seq.h — many sequences of dependent comprop blocks coded in lockstep (crgpu_model_set,
 * crgpu_encode_sequences_carried*).
 *
 * crgpu_carry.h codes ONE chain of dependent blocks, and one block gives k_rop_rc, the event kernel and the sorts one
 * workgroup each. The parallel work that is missing is other sequences: step t of a call codes block t of every sequence
 * that has one. The host orders the sequences by block count, descending, so the active set of a step is a prefix, and lays
 * the block descriptors out step-major: the pre-pass (k_rop_lzp*), the sorts (k_rop_links*) and the range coder (k_rop_rc)
 * of crgpu.hip run unchanged on the step's sub-batch. The kernels here are the model-dependent ones, each launched ONCE per
 * step for all active blocks:
 *
 *   k_seq_fill     the ppm_model_init state in any subset of slots
 *   k_seq_gather   block descriptors from the caller's order into the step-major one; k_seq_scatter takes the sizes back
 *   k_seq_events   one wave per active block; the context register comes from and goes back to the block's slot
 *   k_seq_o3       one lane per order-3 chain. The grid is split by block (blockIdx.y = active block), not by a flattened
 *                  chain index: the chain counts are only known on the device (ctr[2] of every block), a flat index would
 *                  need a prefix sum over the blocks and a search per lane, and a block's chains are walked through the
 *                  block's own views anyway. blockIdx.x strides over the block's chains as k_ropc_o3's grid does.
 *   k_seq_o2       one lane per order-2 chain, the node in the lane's LDS slice (cr_ropc_o2_all); chains handed out from
 *                  one counter per active block, an array of its own in device memory
 *   k_seq_o1       cr_rop_o1_all per active block on its slot's rows
 *   k_seq_undo     for a block that ended stored: the models go back to where they stood in front of the block
 *
 * STORE: one allocation of nseq x CR_M_BYTES, slot s at s * CR_M_BYTES, every slot laid out as crgpu_carry.h says.
 *
 * UNDO LOG instead of a second store and a store-sized copy per block. A chain loads its start state anyway; it also
 * writes it to the log of its slot, and k_seq_undo writes the log back. Per slot, E = the event capacity of a block of the
 * set's max_block bytes (align_up(max(max_block, 1024) + max_block / 64 + 128, 64), the ev_cap of every encode launch):
 *   the 65 536 order-1 bytes and the register, written by k_seq_events at entry          65 536 + 256 = 65 792
 *   order-2: {256 old counts, old flag word, context} per chain, 280 bytes a record      280 x min(E, 65 536)
 *            (the counts only if the record had any; a block has no more chains than contexts)
 *   order-3: {key, old cell} per chain                                                   8 x min(E, 1 << 22)
 *                                                     = 65 792 + 280 x min(E, 65 536) + 8 x min(E, 1 << 22) bytes
 * (18.9 MB for 64 KiB blocks — against 26.3 MB of a second store, and written and read only where chains start: ~1 MB a
 * block of text instead of 2 x 26.3 MB.) The chains of a block never share a cell, so the order of the write-back is free.
 */
#ifndef CRGPU_SEQ_H
#define CRGPU_SEQ_H

#include "crgpu_carry.h"

#define CR_SEQ_LOG1_BYTES 65792ull         /* order-1 rows, then the register in a 256-byte tail */
#define CR_SEQ_LOG2_REC   280u             /* counts 0..255, flag word 256, context 260 */

struct CrSeq {
    uint8_t*        store;      /* slot s at store + s * CR_M_BYTES */
    uint8_t*        log;        /* slot s at log + s * log_stride: order-1 + register, order-2 records at CR_SEQ_LOG1_BYTES, order-3 at off_log3 */
    u64             log_stride;
    u64             off_log3;
    const uint32_t* slot;       /* the slot of every active block of the launch */
    uint32_t*       chain_ctr;  /* one word per active block: the next order-2 chain to hand out */
};

/* launchers (crgpu_seq.hip); B describes the launch's blocks: every per-block pointer moved on to its first, nblocks of them */
void crs_launch_fill(hipStream_t s, uint32_t grid, uint8_t* store, const uint32_t* which, uint32_t n);
void crs_launch_gather(hipStream_t s, const uint32_t* map, uint32_t n, const u64* in_off, const uint32_t* in_size, const u64* out_off,
                       u64* d_in_off, uint32_t* d_in_size, u64* d_out_off);
void crs_launch_scatter(hipStream_t s, const uint32_t* map, uint32_t n, const uint32_t* d_out_size, uint32_t* out_size);
void crs_launch_events(hipStream_t s, const CrBatch& B, const CrArenaLayout& L, const CrSeq& Q);
void crs_launch_o3(hipStream_t s, uint32_t grid_x, const CrBatch& B, const CrSeq& Q);
void crs_launch_o2(hipStream_t s, uint32_t grid_x, const CrBatch& B, const CrSeq& Q);
void crs_launch_o1(hipStream_t s, const CrBatch& B, const CrSeq& Q);
void crs_launch_undo(hipStream_t s, const CrBatch& B, const CrSeq& Q);

#ifdef CRGPU_SEQ_TU

CR_DEV uint8_t* cr_seq_slot(const CrSeq& Q, uint32_t j) { return Q.store + (u64)Q.slot[j] * CR_M_BYTES; }
CR_DEV uint8_t* cr_seq_log(const CrSeq& Q, uint32_t j) { return Q.log + (u64)Q.slot[j] * Q.log_stride; }

/* k_ropc_fill for the slots which[0 .. gridDim.y) (which == nullptr: slot y) */
__global__ __launch_bounds__(256) void k_seq_fill(uint8_t* store, const uint32_t* which) {
    uint8_t* const M = store + (u64)(which ? which[blockIdx.y] : blockIdx.y) * CR_M_BYTES;
    const u64 words = CR_M_BYTES / 16u;
    for (u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (u64)gridDim.x * blockDim.x) {
        const u64 o = w * 16u;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (o < CR_M_OFF_O2) v = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
        else if (o < CR_M_OFF_O3 && (o - CR_M_OFF_O2) % CR_M_O2_REC == 256u) v.x = 0x0101u;
        reinterpret_cast<uint4*>(M)[w] = v;
    }
}

/* position p of the step-major order is the caller's block map[p]; only descriptors move */
__global__ __launch_bounds__(256) void k_seq_gather(const uint32_t* map, uint32_t n, const u64* in_off, const uint32_t* in_size, const u64* out_off,
                                                    u64* d_in_off, uint32_t* d_in_size, u64* d_out_off) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t b = map[p];
    d_in_off[p] = in_off[b]; d_in_size[p] = in_size[b]; d_out_off[p] = out_off[b];
}
__global__ __launch_bounds__(256) void k_seq_scatter(const uint32_t* map, uint32_t n, const uint32_t* d_out_size, uint32_t* out_size) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) out_size[map[p]] = d_out_size[p];
}

/* k_ropc_events for block blockIdx.x of the step. A block of 16 bytes or more may end stored: what k_seq_undo cannot take
 * from a chain's log — the order-1 rows (every row may move) and the register — is logged here, 1 KiB per wave step */
__global__ __launch_bounds__(CRGPU_WAVE) void k_seq_events(CrBatch B, CrArenaLayout L, CrSeq Q) {
    __shared__ CrShared sh;
    const uint32_t j = blockIdx.x;
    const uint32_t n = B.in_size[j];
    CrEvViews V = cr_ev_views(B.ev + (u64)j * B.ev_stride, B.ev_cap);
    uint8_t* const M = cr_seq_slot(Q, j);
    uint32_t* const ctx = reinterpret_cast<uint32_t*>(M + CR_M_OFF_CTX);
    if (n > L.max_block) {
        if (threadIdx.x == 0) { V.ctr[0] = 0; V.ctr[1] = 0; V.ctr[2] = 0; V.ctr[3] = 0x200u; }
        return;
    }
    if (n >= 16u) {
        const uint4* const from = reinterpret_cast<const uint4*>(M + CR_M_OFF_O1);
        uint4* const to = reinterpret_cast<uint4*>(cr_seq_log(Q, j));
        for (uint32_t w = threadIdx.x; w < 4096u; w += 4u * CRGPU_WAVE) {
            uint4 v[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) v[u] = from[w + u * CRGPU_WAVE];
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) to[w + u * CRGPU_WAVE] = v[u];
        }
        if (threadIdx.x == 0) reinterpret_cast<uint32_t*>(to + 4096u)[0] = *ctx;
    }
    cr_rop_emit_events<true>(B.in + B.in_off[j], n, B.lens + (u64)j * B.lens_stride, V, sh, ctx);
    if (threadIdx.x == 0) V.ctr[CR_CTR_END_CTX] = *ctx;
}

/* k_ropc_o3 for block blockIdx.y; a lane that starts a chain logs {key, old cell}. The first workgroup of a block also
 * puts the block's order-2 chain counter back to 0 for the kernel behind this one */
__global__ __launch_bounds__(256) void k_seq_o3(CrBatch B, CrSeq Q) {
    const uint32_t j = blockIdx.y;
    CrEvViews V = cr_ev_views(B.ev + (u64)j * B.ev_stride, B.ev_cap);
    const uint32_t nev = V.ctr[0];
    const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x, gn = gridDim.x * blockDim.x;
    if (gt == 0u) Q.chain_ctr[j] = 0u;
    for (uint32_t i = gt * 2u; i < nev; i += gn * 2u) { const u64 f = CR_TRIP_FRESH; *reinterpret_cast<ulonglong2*>(V.trip + i) = make_ulonglong2(f, f); }
    const uint32_t nc = nev ? V.ctr[2] : 0u;
    uint16_t* const o3 = reinterpret_cast<uint16_t*>(cr_seq_slot(Q, j) + CR_M_OFF_O3);
    uint2* const log3 = reinterpret_cast<uint2*>(cr_seq_log(Q, j) + Q.off_log3);
    for (uint32_t c = gt; c < nc; c += gn) cr_ropc_o3_chain<true>(V, o3, V.starts3[c], log3 + c);
}

/* k_ropc_o2 for block blockIdx.y: the workgroups of a block share the block's counter, chain h logs into record h */
__global__ __launch_bounds__(CR_O2C_THREADS) void k_seq_o2(CrBatch B, CrSeq Q) {
    __shared__ __attribute__((aligned(16))) uint8_t s_nodes[CR_O2C_THREADS * CR_LN_STRIDE];
    const uint32_t j = blockIdx.y;
    CrEvViews V = cr_ev_views(B.ev + (u64)j * B.ev_stride, B.ev_cap);
    const uint32_t nev = V.ctr[0];
    const uint32_t nc = nev ? V.ctr[1] : 0u;
    cr_ropc_o2_all<true>(V, s_nodes + threadIdx.x * CR_LN_STRIDE, cr_seq_slot(Q, j) + CR_M_OFF_O2, nc, Q.chain_ctr + j, cr_seq_log(Q, j) + CR_SEQ_LOG1_BYTES);
}

__global__ __launch_bounds__(CR_O1_THREADS) void k_seq_o1(CrBatch B, CrSeq Q) {
    __shared__ CrSortShared sh;
    static_assert(sizeof(sh.buf) >= CR_SORT_WAVES * CR_O1_LDS_PER_WAVE * 4u, "the order-1 rows' LDS lies over the sort tile");
    uint32_t* const s_masks = reinterpret_cast<uint32_t*>(sh.buf);
    const uint32_t j = blockIdx.x;
    CrEvViews V = cr_ev_views(B.ev + (u64)j * B.ev_stride, B.ev_cap);
    const uint32_t nev = (V.ctr[3] & 0x300u) ? 0u : V.ctr[0];
    if (nev) cr_rop_o1_all(sh, V, s_masks, nev, B.o2_tickets, nullptr, cr_seq_slot(Q, j) + CR_M_OFF_O1);
}

/* One workgroup per block that ended stored, before anything sorts the block's events again (ctr[1] and ctr[2] still count
 * the chains that were walked and logged): the order-1 rows and the register, the order-2 record of every chain — a record
 * that held no byte goes back to zeros, as k_seq_fill and cr_ln_save keep such records —, the order-3 cell of every chain.
 * k_ropc_abort then cuts the event list and sets the register; the chain kernels run again over the cut list */
__global__ __launch_bounds__(256) void k_seq_undo(CrBatch B, CrSeq Q) {
    const uint32_t j = blockIdx.x;
    CrEvViews V = cr_ev_views(B.ev + (u64)j * B.ev_stride, B.ev_cap);
    uint8_t* const M = cr_seq_slot(Q, j);
    const uint8_t* const lg = cr_seq_log(Q, j);
    if ((V.ctr[3] & 0x300u) || V.ctr[0] == 0u) return;
    for (uint32_t w = threadIdx.x; w < 4096u; w += blockDim.x) reinterpret_cast<uint4*>(M + CR_M_OFF_O1)[w] = reinterpret_cast<const uint4*>(lg)[w];
    if (threadIdx.x == 0) *reinterpret_cast<uint32_t*>(M + CR_M_OFF_CTX) = *reinterpret_cast<const uint32_t*>(lg + 65536u);
    const uint32_t nc2 = V.ctr[1], nc3 = V.ctr[2];
    const uint32_t lane = cr_lane();
    for (uint32_t h = cr_wave_id(); h < nc2; h += blockDim.x / CRGPU_WAVE) {
        const uint8_t* const r = lg + CR_SEQ_LOG1_BYTES + (u64)h * CR_SEQ_LOG2_REC;
        const uint2 fc = *reinterpret_cast<const uint2*>(r + 256u);                       /* flag word, context */
        uint8_t* const rec = M + CR_M_OFF_O2 + (u64)(fc.y & 0xffffu) * CR_M_O2_REC;
        if (lane < 32u) reinterpret_cast<uint2*>(rec)[lane] = (fc.x >> 16) ? reinterpret_cast<const uint2*>(r)[lane] : make_uint2(0u, 0u);
        else if (lane == 32u) *reinterpret_cast<uint32_t*>(rec + 256u) = fc.x;
    }
    uint16_t* const o3 = reinterpret_cast<uint16_t*>(M + CR_M_OFF_O3);
    const uint2* const log3 = reinterpret_cast<const uint2*>(lg + Q.off_log3);
    for (uint32_t c = threadIdx.x; c < nc3; c += blockDim.x) { const uint2 kc = log3[c]; o3[kc.x & 0x3fffffu] = (uint16_t)kc.y; }
}

#endif /* CRGPU_SEQ_TU */
#endif
