/*
 * comprox_amd/csrc/crgpu_dicpick.h — the whole-stream word census that picks the static dictionary
 * (reference src/cr-dicpick.c:164-259), on the device.
 *
 * The top of this file is plain C: the (text, hits) cell and the tail that turns the kept cells into
 * the dictionary text, shared with the host census in crhost_dict.c. The kernels follow for hipcc.
 *
 *   k_dic_scan<false>  tiles of 8 192 bytes through LDS, 64 bytes per ballot: token count per tile
 *   k_dic_offsets      exclusive sum of the tile counts
 *   k_dic_scan<true>   the same walk, writing the tokens {pos, hash} in stream order
 *   k_dic_insert       lane per token: word -> slot of an open-addressing table (one 64-bit CAS), total hits
 *   k_dic_first / k_dic_flags / k_dic_select / k_dic_count / k_dic_min / k_dic_purge
 *                      the replay of the reference's "forget the little-used words" purge, one epoch per purge
 *   k_dic_keep         live words with more than 5 hits -> (text, hits) cells for the host tail
 */
#ifndef CRGPU_DICPICK_H
#define CRGPU_DICPICK_H

#include "../../include/crgpu.h"

#define CR_DIC_WORD_MIN   2u
#define CR_DIC_WORD_MAX   20u
#define CR_DIC_FULL       (25000u * 13u + 1u)       /* live words at which the purge fires, cr-dicpick.c:33,115 */
#define CR_DIC_KEEP_ABOVE 5u                        /* cr-dicpick.c:35; also the purge's margin (:132)          */
#define CR_DIC_CHUNK      200000u                   /* cr-dicpick.c:162                                         */

typedef struct { char text[CR_DIC_WORD_MAX + 1]; int hits; } crh_cell;

#ifdef __cplusplus
extern "C"
#endif
/* cr-dicpick.c:227-257: `kept` cells with distinct lower-cased texts and hits > 5, in any order (both sorts are total
 * orders on distinct texts) -> the dictionary text appended to dic_block. `live` only sizes the reservation (:239). */
void crh_dict_tail(crh_cell* cells, int kept, int live, data_block_t* dic_block);

#ifdef __HIPCC__
#include "crgpu_wave.h"

#define CR_DIC_TILE     8192u                       /* bytes per workgroup of k_dic_scan */
#define CR_DIC_THREADS  256u
#define CR_DIC_GROUPS   (CR_DIC_TILE / 64u)         /* 64-byte ballot groups per tile */
#define CR_DIC_SPAN     (CR_DIC_GROUPS / (CR_DIC_THREADS / 64u))   /* groups per wave */
#define CR_DIC_HALO     64u                         /* one group in front (the byte before a start) and one behind (a word's
                                                       <= 19 further letters and its closing byte: 21 bytes are needed) */
#define CR_DIC_BLK      1024u                       /* tokens per workgroup of the replay's scans */
/* the chunk length is a multiple of the group length: a chunk's zeroed last byte is always lane 63 of a group, its
 * offset 0 always lane 0, and no token crosses from one chunk into the next */
static_assert(CR_DIC_CHUNK % 64u == 0u && CR_DIC_TILE % 64u == 0u && CR_DIC_HALO % 16u == 0u, "k_dic_scan's chunk rules");

struct CrDicTok { uint32_t pos, hash; };
/* device state of one census: what the host reads back to steer */
enum { CR_DS_TOKENS = 0, CR_DS_DISTINCT, CR_DS_LIVE, CR_DS_FOUND, CR_DS_POINT, CR_DS_NEW, CR_DS_MIN, CR_DS_KEPT, CR_DS_LIVE_WAS, CR_DS_WORDS };

struct CrDic {
    const uint8_t* src;
    u64            n;
    uint32_t*      tile_cnt;    /* per tile: tokens, then (k_dic_offsets) tokens in front of the tile */
    uint32_t       ntiles;
    uint32_t*      st;          /* CR_DS_* */
    CrDicTok*      toks;        /* stream order; the same bytes later hold `first`, then the kept cells */
    uint32_t       ntok;
    uint32_t*      slot_of;     /* token -> slot */
    u64*           table;       /* slot -> {hash:32, pos:32} of the word's first claimant, 0 = empty (pos >= 1 always) */
    uint32_t       nslots;
    uint32_t*      hits;        /* slot -> hits; in the replay 0 = not live, as in the reference's map */
    uint32_t*      first;       /* replay: slot -> first token of the epoch that holds the word, 0xFFFFFFFF = none */
    uint32_t*      blk_cnt;     /* replay: epoch-first tokens per CR_DIC_BLK tokens */
    crh_cell*      cells;
};

CR_DEV bool cr_dic_lower(uint32_t c) { return c - 'a' < 26u; }
CR_DEV bool cr_dic_letter(uint32_t c) { return (c | 32u) - 'a' < 26u; }
CR_DEV bool cr_dic_closer(uint32_t c) { return c == ' ' || c == ',' || c == '.' || c == ':' || c == ';'; }

/* the byte the reference's loop sees at stream position pos: the last byte of every 200 000-byte chunk, and of the
 * stream, reads as 0 (cr-dicpick.c:192); s_b holds the raw bytes of [tile - HALO, tile + TILE + HALO), 0 outside the stream */
CR_DEV uint32_t cr_dic_seen(const uint8_t* s_b, u64 tile_base, u64 n, int group, uint32_t lane) {
    const long long pos = (long long)tile_base + (long long)group * 64 + (long long)lane;
    const uint32_t behind = (uint32_t)(tile_base / 64u) + (uint32_t)(group + 1);          /* groups up to and with this one */
    if (pos + 1 == (long long)n || (lane == 63u && behind % (CR_DIC_CHUNK / 64u) == 0u)) return 0u;
    return s_b[(int)CR_DIC_HALO + group * 64 + (int)lane];
}

/* FILL = false: tile_cnt[tile] = tokens of the tile. FILL = true: tile_cnt holds the exclusive sums; the tokens are
 * written at their rank in stream order. Grid = tiles, 256 threads: each wave walks CR_DIC_SPAN consecutive groups with
 * the masks of the group behind the current one in hand. */
template <bool FILL>
__global__ __launch_bounds__(CR_DIC_THREADS) void k_dic_scan(CrDic D) {
    __shared__ __attribute__((aligned(16))) uint8_t s_b[CR_DIC_HALO + CR_DIC_TILE + CR_DIC_HALO];
    __shared__ u64 s_acc[CR_DIC_GROUPS];
    __shared__ uint32_t s_wave[CR_DIC_THREADS / 64u];
    const u64 base = (u64)blockIdx.x * CR_DIC_TILE;
    for (uint32_t i = threadIdx.x; i < sizeof s_b / 16u; i += CR_DIC_THREADS) {
        const long long p = (long long)base - (long long)CR_DIC_HALO + (long long)i * 16;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (p >= 0 && (u64)p + 16u <= D.n) __builtin_memcpy(&v, D.src + p, 16);
        else if (p >= 0 && (u64)p < D.n) {                            /* the stream's last, partial piece */
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t k = 0; k < 16u; k++) if ((u64)p + k < D.n) w[k >> 2] |= (uint32_t)D.src[p + k] << (8u * (k & 3u));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(s_b + i * 16u) = v;
    }
    __syncthreads();
    const uint32_t lane = cr_lane(), wave = cr_wave_id();
    const int g0 = (int)(wave * CR_DIC_SPAN);
    u64 before = cr_ballot(cr_dic_letter(cr_dic_seen(s_b, base, D.n, g0 - 1, lane)));
    uint32_t c = cr_dic_seen(s_b, base, D.n, g0, lane);
    u64 letter = cr_ballot(cr_dic_letter(c)), lower = cr_ballot(cr_dic_lower(c)), closer = cr_ballot(cr_dic_closer(c));
    uint32_t count = 0;
    for (int g = g0; g < g0 + (int)CR_DIC_SPAN; g++) {
        c = cr_dic_seen(s_b, base, D.n, g + 1, lane);
        const u64 letter1 = cr_ballot(cr_dic_letter(c)), lower1 = cr_ballot(cr_dic_lower(c)), closer1 = cr_ballot(cr_dic_closer(c));
        /* a word starts at a letter behind a non-letter, never at offset 0 of a chunk (x = 1, cr-dicpick.c:193,197) */
        u64 starts = letter & ~((letter << 1) | (before >> 63));
        if (((uint32_t)(base / 64u) + (uint32_t)g) % (CR_DIC_CHUNK / 64u) == 0u) starts &= ~1ull;
        /* the 64 bytes behind this lane's: lower-case run = the word's further letters, then the closing byte (:199-203) */
        const u64 low = ((lower >> lane) >> 1) | (lower1 << (63u - lane));
        const u64 clo = ((closer >> lane) >> 1) | (closer1 << (63u - lane));
        const uint32_t run = ~low ? (uint32_t)__builtin_ctzll(~low) : 64u;
        const bool ok = ((starts >> lane) & 1ull) && run + 1u >= CR_DIC_WORD_MIN && run + 1u <= CR_DIC_WORD_MAX && ((clo >> run) & 1ull);
        const u64 acc = cr_ballot(ok);
        count += (uint32_t)__builtin_popcountll(acc);
        if (FILL && lane == 0u) s_acc[g] = acc;
        before = letter; letter = letter1; lower = lower1; closer = closer1;
    }
    if (lane == 0u) s_wave[wave] = count;
    __syncthreads();
    if (!FILL) {
        if (threadIdx.x == 0u) D.tile_cnt[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        return;
    }
    uint32_t at = D.tile_cnt[blockIdx.x];
    for (uint32_t w = 0; w < wave; w++) at += s_wave[w];
    for (int g = g0; g < g0 + (int)CR_DIC_SPAN; g++) {
        const u64 acc = s_acc[g];
        if ((acc >> lane) & 1ull) {
            /* an accepted word ends in front of its chunk's last byte: the raw bytes are what the reference saw */
            const uint8_t* w = s_b + CR_DIC_HALO + (uint32_t)g * 64u + lane;
            uint32_t h = w[0] | 32u;                                 /* cr-dicpick.c:70-77, over the lower-cased letters */
            for (uint32_t k = 1; k < CR_DIC_WORD_MAX && cr_dic_lower(w[k]); k++) h = h * 131313131u + w[k];
            CrDicTok t;
            t.pos = (uint32_t)(base + (u64)g * 64u + lane);
            t.hash = h & 0x7fffffffu;
            D.toks[at + (uint32_t)__builtin_popcountll(acc & ((1ull << lane) - 1ull))] = t;
        }
        at += (uint32_t)__builtin_popcountll(acc);
    }
}

/* inclusive sum over a workgroup of 1024 threads; *total = the sum. s_wave: 16 words of LDS */
CR_DEV uint32_t cr_dic_scan1024(uint32_t v, uint32_t* s_wave, uint32_t* total) {
    uint32_t incl = cr_scan_incl(v);
    __syncthreads();                                                 /* s_wave may still be read from the previous call */
    if (cr_lane() == 63u) s_wave[cr_wave_id()] = incl;
    __syncthreads();
    uint32_t sum = 0;
    for (uint32_t k = 0; k < CR_DIC_BLK / 64u; k++) { if (k < cr_wave_id()) incl += s_wave[k]; sum += s_wave[k]; }
    *total = sum;
    return incl;
}

/* tile_cnt: counts -> exclusive sums, st[CR_DS_TOKENS] = the total. One workgroup of 1024 threads. */
__global__ __launch_bounds__(CR_DIC_BLK) void k_dic_offsets(CrDic D) {
    __shared__ uint32_t s_wave[CR_DIC_BLK / 64u];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < D.ntiles; base += CR_DIC_BLK) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t v = t < D.ntiles ? D.tile_cnt[t] : 0u;
        uint32_t total;
        const uint32_t incl = cr_dic_scan1024(v, s_wave, &total);
        if (t < D.ntiles) D.tile_cnt[t] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0u) D.st[CR_DS_TOKENS] = carry;
}

/* the same word? Both positions hold counted words: a letter, lower-case letters, a closing byte inside the stream
 * (cr-dicpick.c:78-87 on such words) */
CR_DEV bool cr_dic_same_word(const uint8_t* src, uint32_t a, uint32_t b) {
    if (a == b) return true;
    if ((src[a] | 32u) != (src[b] | 32u)) return false;
    for (uint32_t k = 1; k <= CR_DIC_WORD_MAX; k++) {
        const uint32_t ca = src[(u64)a + k], cb = src[(u64)b + k];
        const bool la = cr_dic_lower(ca), lb = cr_dic_lower(cb);
        if (!la || !lb) return la == lb;
        if (ca != cb) return false;
    }
    return true;
}

/* hits[slot] += 1 for every active lane, one atomic per distinct slot of the wave. All 64 lanes call. */
CR_DEV void cr_dic_add_hits(uint32_t* hits, uint32_t slot, bool active) {
    u64 todo = cr_ballot(active);
    while (todo) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t s = cr_lane_get(slot, leader);
        const u64 same = cr_ballot(active && slot == s);
        if (cr_lane() == leader) atomicAdd(&hits[s], (uint32_t)__builtin_popcountll(same));
        todo &= ~same;
    }
}

/* One lane per token: walk the table from the hash's home slot to the word's slot — an empty slot is claimed by one
 * 64-bit compare-and-swap of {hash, pos}, a slot with the same hash is the word's if the letters at its pos are the
 * same. Every step ends the walk or moves on: nobody waits for anybody. Also the totals: hits per slot, distinct words. */
__global__ __launch_bounds__(CR_DIC_THREADS) void k_dic_insert(CrDic D) {
    const uint32_t i = blockIdx.x * CR_DIC_THREADS + threadIdx.x;
    const bool active = i < D.ntok;
    uint32_t s = 0;
    bool claimed = false;
    if (active) {
        const CrDicTok t = D.toks[i];
        const u64 mine = ((u64)t.hash << 32) | t.pos;
        s = (uint32_t)(((u64)(t.hash * 0x9E3779B1u) * D.nslots) >> 32);
        for (;;) {
            u64 e = cr_ld64(&D.table[s]);
            if (e == 0ull) {
                e = atomicCAS(&D.table[s], 0ull, mine);
                if (e == 0ull) { claimed = true; break; }
            }
            if ((uint32_t)(e >> 32) == t.hash && cr_dic_same_word(D.src, (uint32_t)e, t.pos)) break;
            if (++s == D.nslots) s = 0;
        }
        D.slot_of[i] = s;
    }
    cr_dic_add_hits(D.hits, s, active);
    const u64 fresh = cr_ballot(claimed);
    if (cr_lane() == 0u && fresh) atomicAdd(&D.st[CR_DS_DISTINCT], (uint32_t)__builtin_popcountll(fresh));
}

__global__ __launch_bounds__(CR_DIC_THREADS) void k_dic_fill32(uint32_t* p, uint32_t count, uint32_t value) {
    for (uint32_t i = blockIdx.x * CR_DIC_THREADS + threadIdx.x; i < count; i += gridDim.x * CR_DIC_THREADS) p[i] = value;
}

/* ---- the purge, replayed. An epoch starts behind a purge (or at token 0) at token `from` with the live words = the
 * slots with hits > 0. Until the next purge the reference's map only grows, by one word at the first token of every
 * word that is not live; the purge fires at the token whose insertion is the (CR_DIC_FULL - live)-th of the epoch. ---- */

/* first[slot] = the first token from `from` on that holds the slot's word, for the words that are not live */
__global__ __launch_bounds__(CR_DIC_THREADS) void k_dic_first(CrDic D, uint32_t from) {
    const uint32_t i = from + blockIdx.x * CR_DIC_THREADS + threadIdx.x;
    if (i >= D.ntok) return;
    const uint32_t s = D.slot_of[i];
    if (D.hits[s] == 0u && cr_ld32(&D.first[s]) > i) atomicMin(&D.first[s], i);
}

/* blk_cnt[b] = insertions among the tokens [from + b * BLK, + BLK) */
__global__ __launch_bounds__(CR_DIC_BLK) void k_dic_flags(CrDic D, uint32_t from) {
    __shared__ uint32_t s_wave[CR_DIC_BLK / 64u];
    const u64 i = (u64)from + (u64)blockIdx.x * CR_DIC_BLK + threadIdx.x;
    const bool ins = i < D.ntok && D.first[D.slot_of[i]] == (uint32_t)i;
    const uint32_t cnt = (uint32_t)__builtin_popcountll(cr_ballot(ins));
    if (cr_lane() == 0u) s_wave[cr_wave_id()] = cnt;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t sum = 0;
        for (uint32_t k = 0; k < CR_DIC_BLK / 64u; k++) sum += s_wave[k];
        D.blk_cnt[blockIdx.x] = sum;
    }
}

/* The token at which the running number of insertions reaches CR_DIC_FULL - live: st[FOUND] = 1, st[POINT] = the token;
 * or st[FOUND] = 0 and st[NEW] = the insertions up to the stream's end. One workgroup: the block counts first, then the
 * tokens of the block that crosses. Leaves st[MIN] and st[LIVE] ready for k_dic_min / k_dic_purge to accumulate into. */
__global__ __launch_bounds__(CR_DIC_BLK) void k_dic_select(CrDic D, uint32_t from, uint32_t nblk) {
    __shared__ uint32_t s_wave[CR_DIC_BLK / 64u];
    __shared__ uint32_t s_blk, s_before;
    const uint32_t live = D.st[CR_DS_LIVE];
    const uint32_t need = CR_DIC_FULL - live;
    if (threadIdx.x == 0u) s_blk = 0xFFFFFFFFu;
    __syncthreads();
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nblk; base += CR_DIC_BLK) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < nblk ? D.blk_cnt[b] : 0u;
        uint32_t total;
        const uint32_t incl = carry + cr_dic_scan1024(v, s_wave, &total);
        if (incl >= need && incl - v < need) { s_blk = b; s_before = incl - v; }
        carry += total;
        __syncthreads();
        if (s_blk != 0xFFFFFFFFu) break;
    }
    const uint32_t blk = s_blk;
    if (blk != 0xFFFFFFFFu) {
        const u64 i = (u64)from + (u64)blk * CR_DIC_BLK + threadIdx.x;
        const bool ins = i < D.ntok && D.first[D.slot_of[i]] == (uint32_t)i;
        uint32_t total;
        const uint32_t incl = s_before + cr_dic_scan1024(ins ? 1u : 0u, s_wave, &total);
        if (ins && incl == need) { D.st[CR_DS_FOUND] = 1u; D.st[CR_DS_POINT] = (uint32_t)i; D.st[CR_DS_NEW] = need; }
    } else if (threadIdx.x == 0u) { D.st[CR_DS_FOUND] = 0u; D.st[CR_DS_NEW] = carry; }
    if (threadIdx.x == 0u) { D.st[CR_DS_LIVE_WAS] = live; D.st[CR_DS_MIN] = 0xFFFFFFFFu; D.st[CR_DS_LIVE] = 0u; }
}

/* hits of the tokens [from, to] */
__global__ __launch_bounds__(CR_DIC_THREADS) void k_dic_count(CrDic D, uint32_t from, uint32_t to) {
    const u64 i = (u64)from + (u64)blockIdx.x * CR_DIC_THREADS + threadIdx.x;
    const bool active = i <= to;
    cr_dic_add_hits(D.hits, active ? D.slot_of[i] : 0u, active);
}

/* st[MIN] = the fewest hits of a live word (cr-dicpick.c:117-123; 1, the word whose insertion fired the purge) */
__global__ __launch_bounds__(CR_DIC_THREADS) void k_dic_min(CrDic D) {
    uint32_t m = 0xFFFFFFFFu;
    for (uint32_t s = blockIdx.x * CR_DIC_THREADS + threadIdx.x; s < D.nslots; s += gridDim.x * CR_DIC_THREADS) {
        const uint32_t h = D.hits[s];
        if (h != 0u && h < m) m = h;
    }
    for (uint32_t d = 32; d; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)m, (int)d, 64); if (o < m) m = o; }
    if (cr_lane() == 0u && m != 0xFFFFFFFFu) atomicMin(&D.st[CR_DS_MIN], m);
}

/* cr-dicpick.c:131-142: every word within 5 hits of the minimum is forgotten, the others keep their hits; st[LIVE] = the
 * survivors. `first` is cleared for the next epoch. */
__global__ __launch_bounds__(CR_DIC_THREADS) void k_dic_purge(CrDic D) {
    const uint32_t floor_hits = D.st[CR_DS_MIN];
    uint32_t kept = 0;
    for (uint32_t s = blockIdx.x * CR_DIC_THREADS + threadIdx.x; s < D.nslots; s += gridDim.x * CR_DIC_THREADS) {
        const uint32_t h = D.hits[s];
        if (h != 0u) { if (h - floor_hits <= CR_DIC_KEEP_ABOVE) D.hits[s] = 0u; else kept++; }
        D.first[s] = 0xFFFFFFFFu;
    }
    kept = cr_sum(kept);
    if (cr_lane() == 0u && kept) atomicAdd(&D.st[CR_DS_LIVE], kept);
}

/* cr-dicpick.c:219-226: the words with more than 5 hits, lower-cased, as cells in any order; st[KEPT] = their number */
__global__ __launch_bounds__(CR_DIC_THREADS) void k_dic_keep(CrDic D) {
    for (uint32_t base = blockIdx.x * CR_DIC_THREADS; base < D.nslots; base += gridDim.x * CR_DIC_THREADS) {
        const uint32_t s = base + threadIdx.x;
        const uint32_t h = s < D.nslots ? D.hits[s] : 0u;
        const bool keep = h > CR_DIC_KEEP_ABOVE;
        const u64 m = cr_ballot(keep);
        if (!m) continue;
        uint32_t at = 0;
        if (cr_lane() == 0u) at = atomicAdd(&D.st[CR_DS_KEPT], (uint32_t)__builtin_popcountll(m));
        at = cr_uni(at) + (uint32_t)__builtin_popcountll(m & ((1ull << cr_lane()) - 1ull));
        if (keep) {
            const uint8_t* w = D.src + (uint32_t)D.table[s];
            crh_cell c;
            uint32_t k = 1;
            c.text[0] = (char)(w[0] | 32u);
            for (; k < CR_DIC_WORD_MAX && cr_dic_lower(w[k]); k++) c.text[k] = (char)w[k];
            for (; k <= CR_DIC_WORD_MAX; k++) c.text[k] = 0;
            c.hits = (int)h;
            D.cells[at] = c;
        }
    }
}

#endif  /* __HIPCC__ */
#endif
