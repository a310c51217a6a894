/*
 * comprox_amd/csrc/crgpu_seq_lz.h — many sequences of dependent comprox / comprolz blocks coded in lockstep: the codec-dependent
 * kernels of a crgpu_model_set made for CRGPU_CODEC_ROX or CRGPU_CODEC_ROLZ.
 *
 * Reference: src/roxmain/cr-coder.c:55-60,88-114,153-318 and src/rolzmain/cr-coder.c:139-264. Between two reset_models() the
 * reference keeps, beside ppm_model and its context register, the small adaptive models of the side streams: len_model,
 * pos_models[6] and spos_model (comprox), len_model and idx_model (comprolz). The matcher, the range coders and the escape byte
 * are the block's own. So a step of crgpu_seq.h changes in two places only: the token loop takes the register and the side
 * models from the sequence's slot and leaves them there, and a block that ends stored goes back to where the token loop gave
 * up — the test runs behind every token, with the header counted (32 / 16 bytes), and there is no size under which a block
 * leaves the models alone: a block of up to header bytes is given up at its first token and moves the models by that token.
 * The match pre-pass (k_rox_links*, k_rox_match, k_rolz_match*), the sorts, k_seq_o3 / _o2 / _o1 / _undo and the range
 * coders k_rox_rc / k_rolz_rc are the kernels the batched encoders and the comprop sets run.
 *
 * KEEP AREA, an allocation of the set beside the PPM stores: per slot two records of CR_SEQ_KEEP_BYTES in cr_side_park's format
 * (u16[8][256] counts, u32[8] totals at byte 4096; comprolz uses models 0 and 1) — the live side models, and their snapshot
 * from in front of the slot's current block, which the abort point starts from.
 *
 *   k_seq_side_fill     the reset_models state of the side models in any subset of slots
 *   k_seq_rox_events    one workgroup of four waves per active block. Wave 0 runs the token loop from the slot's register; in
 *                       its shadow wave 1 takes the snapshot and loads the side models into LDS and waves 2-3 log the order-1
 *                       rows for k_seq_undo. Then waves 0-2 code the three symbol lists on the carried models, side by side (the
 *                       streams share no model), and wave 0 parks the models again
 *   k_seq_rolz_events   one wave per active block: log, snapshot, cr_rolz_emit_events<true> on the slot's register and models
 *   k_seq_lz_abort      one wave, for ONE block that ended stored, behind k_seq_undo: the token at which lzencode gave up
 *                       (cr_ropc_abort_cut with the codec's header), the event list cut there, the register set to the next
 *                       token's context, and the side models = the snapshot plus the side symbols of the tokens up to that one.
 *                       The token loop is not run again: every token that has side symbols is an escape event, so counting the
 *                       escape events of the kept prefix gives the prefix of the length list (comprox) / code list (comprolz),
 *                       and a length says which distance stream its token wrote to and the digits say where a distance ends
 *   k_seq_lz_stored     which blocks of a step came out stored, from the coded flag in their headers (a coded block can have
 *                       a stored block's size by chance); only launched when a size says "maybe"
 */
#ifndef CRGPU_SEQ_LZ_H
#define CRGPU_SEQ_LZ_H

#include "crgpu_seq.h"

#define CR_SEQ_KEEP_BYTES 4352u            /* cr_side_park writes 4128 */
#define CR_SEQ_LZ_END_CTX 13u              /* ctr[13]: the register behind the block's last token (ctr[9] is comprox's) */

/* launchers (crgpu_seq.hip); rolz = 0 comprox, 1 comprolz; B as in crgpu_seq.h, B1 = ONE block */
void crs_launch_side_fill(hipStream_t s, uint8_t* keep, const uint32_t* which, uint32_t n, int rolz);
void crs_launch_lz_events(hipStream_t s, int rolz, const CrBatch& B, const CrArenaLayout& L, const CrSeq& Q, uint8_t* keep);
void crs_launch_lz_abort(hipStream_t s, int rolz, const CrBatch& B1, const CrArenaLayout& L, const CrSeq& Q1, uint8_t* keep);
void crs_launch_lz_stored(hipStream_t s, int rolz, const CrBatch& B, uint32_t* flags);

#ifdef CRGPU_SEQ_TU
#include "crgpu_rox2.h"
#include "crgpu_rolz2.h"

CR_DEV uint8_t* cr_seq_keep(uint8_t* keep, const CrSeq& Q, uint32_t j) { return keep + (u64)Q.slot[j] * 2u * CR_SEQ_KEEP_BYTES; }

/* what the token loops read of a block's match tables: the views cr_rox_tables / cr_rolz_tables_enc of crgpu.hip lay over the
 * block's slot of B.rox (n4 positions: three u32 arrays, then u8 arrays — comprox; two u32 arrays, then rank and length) */
CR_DEV CrRoxTables cr_seq_rox_tables(const CrBatch& B, uint32_t j) {
    CrRoxTables T;
    const u64 n4 = (B.rox_stride / 16u) & ~(u64)63u;
    T.prev = reinterpret_cast<uint32_t*>(B.rox + (u64)j * B.rox_stride);
    T.nprev = T.prev + n4; T.ml_pos = T.nprev + n4;
    T.ml_len = reinterpret_cast<uint8_t*>(T.ml_pos + n4); T.nl_len = T.ml_len + n4; T.m0_len = T.nl_len + n4;
    T.cls_last = nullptr; T.near_last = nullptr;
    return T;
}
CR_DEV CrRolzTables cr_seq_rolz_tables(const CrBatch& B, uint32_t j) {
    CrRolzTables T;
    const u64 n4 = (B.rox_stride / 16u) & ~(u64)63u;
    T.ring_prev = reinterpret_cast<uint32_t*>(B.rox + (u64)j * B.rox_stride);
    T.row_prev = T.ring_prev + n4;
    T.rank = reinterpret_cast<uint8_t*>(T.row_prev + n4); T.len = T.rank + n4;
    T.raw16 = nullptr; T.row16 = nullptr; T.ring16 = nullptr; T.ring_head = nullptr;
    return T;
}

/* reset_models' side models (cr_side_reset / cr_rolz_side_reset; what comprolz does not use is zero) for the slots
 * which[0 .. gridDim.x) (which == nullptr: slot x); the snapshot is written in front of every block */
__global__ __launch_bounds__(CRGPU_WAVE) void k_seq_side_fill(uint8_t* keep, const uint32_t* which, int rolz) {
    __shared__ CrRoxShared sh;
    const uint32_t lane = cr_lane();
    for (uint32_t i = lane; i < 8u * 256u; i += CRGPU_WAVE) sh.f[i >> 8][i & 255u] = 0;
    if (lane < 8u) sh.tot[lane] = 0;
    cr_wave_sync();
    if (rolz) cr_rolz_side_reset(sh); else cr_side_reset(sh);
    cr_wave_sync();
    cr_side_park(sh, keep + (u64)(which ? which[blockIdx.x] : blockIdx.x) * 2u * CR_SEQ_KEEP_BYTES);
}

/* the order-1 rows of a slot into its log, by `nthreads` threads of which this is thread t (k_seq_events' copy) */
CR_DEV void cr_seq_log_o1(const uint8_t* M, uint8_t* lg, uint32_t t, uint32_t nthreads) {
    const uint4* const from = reinterpret_cast<const uint4*>(M + CR_M_OFF_O1);
    uint4* const to = reinterpret_cast<uint4*>(lg);
    for (uint32_t w = t; w < 4096u; w += 4u * nthreads) {
        uint4 v[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) v[u] = from[w + u * nthreads];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) to[w + u * nthreads] = v[u];
    }
}
/* the live side models -> their snapshot, one wave */
CR_DEV void cr_seq_snapshot(uint8_t* K) {
    for (uint32_t i = cr_lane(); i < (4096u + 32u) / 16u; i += CRGPU_WAVE) reinterpret_cast<uint4*>(K + CR_SEQ_KEEP_BYTES)[i] = reinterpret_cast<const uint4*>(K)[i];
}

__global__ __launch_bounds__(256) void k_seq_rox_events(CrBatch B, CrArenaLayout L, CrSeq Q, uint8_t* keep) {
    __shared__ CrRoxShared sh;
    const uint32_t j = blockIdx.x, w = cr_wave_id();
    const uint32_t n = B.in_size[j];
    CrEvViews V = cr_ev_views(B.ev + (u64)j * B.ev_stride, B.ev_cap);
    if (n > L.max_block) {
        if (threadIdx.x == 0) { V.ctr[0] = 0; V.ctr[1] = 0; V.ctr[2] = 0; V.ctr[3] = 0x200u; }
        return;
    }
    uint8_t* const M = cr_seq_slot(Q, j);
    uint8_t* const lg = cr_seq_log(Q, j);
    uint8_t* const K = cr_seq_keep(keep, Q, j);
    uint8_t* const side = B.side + (u64)j * 3u * L.side_stride;
    if (w == 0) {
        uint32_t* const ctx = reinterpret_cast<uint32_t*>(M + CR_M_OFF_CTX);
        if (threadIdx.x == 0) reinterpret_cast<uint32_t*>(lg + 65536u)[0] = *ctx;
        cr_rox_emit_events<true>(B.in + B.in_off[j], n, cr_seq_rox_tables(B, j), side, L.side_stride, V, sh, ctx);
        if (threadIdx.x == 0) V.ctr[CR_SEQ_LZ_END_CTX] = *ctx;
    } else if (w == 1) {
        cr_seq_snapshot(K);
        cr_side_unpark(sh, K);
    } else {
        cr_seq_log_o1(M, lg, threadIdx.x - 2u * CRGPU_WAVE, 2u * CRGPU_WAVE);
    }
    cr_wg_sync_global();
    if (w < 3u) cr_rox_code_side(w, side, L.side_stride, V, sh);
    __syncthreads();
    if (w == 0) cr_side_park(sh, K);
}

/* the code list of a comprolz block: the second third of its side staging (2 n + 256 bytes: a code per token at most) */
CR_DEV uint16_t* cr_seq_rolz_list(const CrBatch& B, const CrArenaLayout& L, uint32_t j) { return reinterpret_cast<uint16_t*>(B.side + ((u64)j * 3u + 1u) * L.side_stride); }

/* a block of 0 bytes touches nothing, one of 1 byte has no token: flushed coders around the slot's untouched state */
__global__ __launch_bounds__(CRGPU_WAVE) void k_seq_rolz_events(CrBatch B, CrArenaLayout L, CrSeq Q, uint8_t* keep) {
    __shared__ CrRoxShared sh;
    const uint32_t j = blockIdx.x;
    const uint32_t n = B.in_size[j];
    CrEvViews V = cr_ev_views(B.ev + (u64)j * B.ev_stride, B.ev_cap);
    if (n > L.max_block) {
        if (threadIdx.x == 0) { V.ctr[0] = 0; V.ctr[1] = 0; V.ctr[2] = 0; V.ctr[3] = 0x200u; }
        return;
    }
    uint8_t* const M = cr_seq_slot(Q, j);
    uint8_t* const K = cr_seq_keep(keep, Q, j);
    uint32_t* const ctx = reinterpret_cast<uint32_t*>(M + CR_M_OFF_CTX);
    if (n != 0u) {
        uint8_t* const lg = cr_seq_log(Q, j);
        cr_seq_log_o1(M, lg, threadIdx.x, CRGPU_WAVE);
        if (threadIdx.x == 0) reinterpret_cast<uint32_t*>(lg + 65536u)[0] = *ctx;
        cr_seq_snapshot(K);
        cr_side_unpark(sh, K);
    }
    cr_rolz_emit_events<true>(B.in + B.in_off[j], n, cr_seq_rolz_tables(B, j), B.side + (u64)j * 3u * L.side_stride, V, sh, ctx, cr_seq_rolz_list(B, L, j));
    if (n != 0u) {
        if (threadIdx.x == 0) V.ctr[CR_SEQ_LZ_END_CTX] = *ctx;
        cr_wave_sync();
        cr_side_park(sh, K);
    }
}

/* how many of the events [0, keep) are escapes: the tokens that put symbols into the side streams */
CR_DEV uint32_t cr_seq_count_esc(const CrEvViews& V, uint32_t keep, uint32_t esc) {
    uint32_t mine = 0;
    for (uint32_t i = cr_lane(); i < keep; i += CRGPU_WAVE) mine += ((uint32_t)V.ev_sym[i] & 0xffu) == esc ? 1u : 0u;
    return cr_uni(cr_sum(mine));
}

template <bool ROLZ>
__global__ __launch_bounds__(CRGPU_WAVE) void k_seq_lz_abort(CrBatch B, CrArenaLayout L, CrSeq Q, uint8_t* keep) {
    __shared__ CrRoxShared sh;
    CrEvViews V = cr_ev_views(B.ev, B.ev_cap);
    const uint32_t n = B.in_size[0];
    const uint32_t nev = cr_uni(V.ctr[0]), info = cr_uni(V.ctr[3]);
    if ((info & 0x700u) || nev == 0u) return;
    const uint32_t kept = cr_ropc_abort_cut(V, n, nev, ROLZ ? CR_ROLZ_HEADER : CR_ROX_HEADER);
    if (cr_lane() == 0) {
        *reinterpret_cast<uint32_t*>(cr_seq_slot(Q, 0) + CR_M_OFF_CTX) = kept < nev ? V.ev_ctx[kept] : V.ctr[CR_SEQ_LZ_END_CTX];
        V.ctr[0] = kept;
    }
    uint8_t* const K = cr_seq_keep(keep, Q, 0);
    cr_side_unpark(sh, K + CR_SEQ_KEEP_BYTES);
    /* (the lists' lengths bound every index below: nothing is read that the token loop did not write) */
    const uint32_t listed = cr_uni(V.ctr[ROLZ ? CR_ROLZC_CODES : CR_ROXC_LIST + 2]);
    uint32_t codes = cr_seq_count_esc(V, kept, info & 0xffu);
    if (codes > listed) codes = listed;
    if constexpr (ROLZ) {
        const uint16_t* const list = cr_seq_rolz_list(B, L, 0);
        for (uint32_t k = 0; k < codes; k++) {
            const uint32_t v = cr_uni((uint32_t)list[k]);
            cr_side_bump(sh, CR_ROLZ_M_LEN, v & 0xffu, 4u);
            if (v & 0xffu) cr_side_bump(sh, CR_ROLZ_M_IDX, v >> 8, 4u);
        }
    } else {
        uint8_t* const side = B.side;
        const u64 side_stride = L.side_stride;
        const uint8_t* const l_spos = CR_ROX_LIST(0);
        const uint16_t* const l_pos = reinterpret_cast<const uint16_t*>(CR_ROX_LIST(1));
        const uint8_t* const l_len = CR_ROX_LIST(2);
        const uint32_t long_min = 10u + (n > 16777216u ? 1u : 0u);
        const uint32_t n_spos = cr_uni(V.ctr[CR_ROXC_LIST + 0]), n_pos = cr_uni(V.ctr[CR_ROXC_LIST + 1]);
        uint32_t i_spos = 0, i_pos = 0;
        for (uint32_t k = 0; k < codes; k++) {                               /* cr-coder.c:235-259,264-267 */
            const uint32_t len = cr_uni((uint32_t)l_len[k]);
            cr_side_bump(sh, CR_SIDE_LEN, len, 30u);
            if (len == 0u) continue;                                         /* a literal escape byte */
            if (len < long_min) { if (i_spos < n_spos) cr_side_bump(sh, CR_SIDE_SPOS, cr_uni((uint32_t)l_spos[i_spos]), 1u); i_spos++; continue; }
            while (i_pos < n_pos) {                                          /* the digits of one distance: the last one is below its base, or the sixth */
                const uint32_t v = cr_uni((uint32_t)l_pos[i_pos]), d = (v >> 8) - CR_SIDE_POS, sym = v & 0xffu;
                i_pos++;
                if (d > 5u) break;
                cr_side_bump(sh, CR_SIDE_POS + d, sym, 1u << (2u * d));
                if (d >= 5u || sym < (d < 2u ? 128u : 64u)) break;
            }
        }
    }
    cr_wave_sync();
    cr_side_park(sh, K);
}

/* flags[j] = 1 where block j of the step is stored: the coded flag is byte 0 of a comprox header, byte 1 of a comprolz one */
__global__ __launch_bounds__(256) void k_seq_lz_stored(CrBatch B, int rolz, uint32_t* flags) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < B.nblocks) flags[j] = B.in_size[j] != 0u && B.out[B.out_off[j] + (rolz ? 1u : 0u)] == 0 ? 1u : 0u;
}

#endif /* CRGPU_SEQ_TU */
#endif
