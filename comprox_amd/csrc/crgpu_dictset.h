/*
 * comprox_amd/csrc/crgpu_dictset.h — the tries of a dictionary SET built on the device: S dictionaries, one per sequence of
 * blocks, made in one call (crgpu_dict_set_create). The host keeps the line parse of dictionary_load (cr-diccode.c:76-106)
 * and uploads the packed words of all dictionaries in one copy; everything from there to the finished `next` / `ids`
 * tables of crgpu_dict.h runs here. The one readback is the node count per dictionary, which sizes the allocation.
 *
 * Memory per dictionary, for as long as the set lives: nnodes x (512 + 4) bytes of trie (a row of 128 links and one id
 * per node; ~40 MB for a dictionary of 25 000 words) plus (nwords + 1) x (24 + 1) bytes of words. All tries of a set are
 * one allocation, all words another. While the set is being built it also holds 13 bytes per word and 4 per node.
 *
 * Node NUMBERS differ from those of the host build (crgpu_dict_create numbers nodes in file order, this one in sorted
 * order); they are internal. The node count, the word numbers and with them every coded byte are the same.
 *
 *   k_dset_sort    one workgroup per dictionary. A stable LSD radix sort of the word numbers (u16) over the 23 byte
 *                  columns, key = (byte & 127) + 1 and 0 past the word's end: the order of the trie's links, a prefix in
 *                  front of its extensions, duplicates in file order. Each of the 16 waves owns a contiguous range; a
 *                  step ranks 64 words among the equal keys of its wave with eight ballots. The two ping-pong arrays stay
 *                  in global memory (50 KB each: they live in L2 next to the 600 KB of words the keys are gathered from),
 *                  which keeps the kernel inside the 64 KB of LDS every workgroup may have without asking. Then the count:
 *                  sorted word j shares lcp_j bytes with its neighbour (six dword compares) and owns len_j - lcp_j new
 *                  nodes, numbered 1 + (exclusive scan) upwards; nnodes = 1 + sum.
 *   k_dset_link    one workgroup per dictionary, depth by depth: a word whose lcp is D walks its first D letters from the
 *                  root over links that the rounds before have finished, hangs its first own node there and chains the
 *                  rest behind it.
 *   k_dset_mark    one thread per word, in file order k: atomicMin(first[node], k) on every node of its path, atomicMax
 *                  (ids[end], k) at its end.
 *   k_dset_ids     one wave per node row. The reference makes a node non-terminal again whenever it gains a NEW child
 *                  later in the file (cr-diccode.c:54-68): with L = the last word that ends at the node and F = the
 *                  largest `first` among its children, its id is L, or -1 when F > L.
 *   k_dset_finish  one wave per node row: the upper-case links of the root ('A'..'Y', cr-diccode.c:107-109), the
 *                  '.' ',' ':' ';' aliases of ' ' where the slot is empty (:110-117), CR_DIC_TERMINAL on links to
 *                  terminal nodes.
 */
#ifndef CRGPU_DICTSET_H
#define CRGPU_DICTSET_H

#include "crgpu_dict.h"

#define CRDS_THREADS 1024u
#define CRDS_WAVES   (CRDS_THREADS / CRGPU_WAVE)
#define CRDS_BINS    129u
#define CRDS_COLS    23u                 /* the longest stored word: 22 bytes and its space (dictionary_load's parse) */
#define CRDS_MAXW    25000u              /* cr-diccode.h:39 */

struct CrDictSetBuild {
    const uint8_t*  words;               /* dictionary s: word_off[s] * 24 onwards, (its words + 1) x 24 bytes, zero padded */
    const uint8_t*  wlen;
    const uint32_t* word_off;            /* ndict + 1 entries: dictionary s owns word_off[s+1] - word_off[s] - 1 words */
    uint16_t*       order0;              /* sort ping-pong; the sorted order ends in order1 (CRDS_COLS is odd) */
    uint16_t*       order1;
    uint8_t*        lcp;                 /* per sorted word */
    uint32_t*       base;                /* per sorted word: nodes owned by the sorted words before it */
    uint32_t*       nnodes;              /* per dictionary, the root included */
    const u64*      node_off;            /* first node of dictionary s within next / ids / first */
    uint32_t*       next;
    int32_t*        ids;
    int32_t*        first;               /* build scratch: the first word (file order) through each node */
    uint32_t        ndict;
};

void crds_launch_sort(hipStream_t s, const CrDictSetBuild& P);
void crds_launch_link(hipStream_t s, const CrDictSetBuild& P);
void crds_launch_mark(hipStream_t s, const CrDictSetBuild& P, uint32_t max_words);
void crds_launch_ids(hipStream_t s, const CrDictSetBuild& P, uint32_t grid_x);
void crds_launch_finish(hipStream_t s, const CrDictSetBuild& P, uint32_t grid_x);

#ifdef CRGPU_DICTSET_TU

CR_DEV uint32_t crds_key(const uint8_t* words, const uint8_t* wlen, uint32_t w, uint32_t col) {
    return col < wlen[w] ? (words[w * CR_DIC_WORD_STRIDE + col] & 127u) + 1u : 0u;
}

/* bytes two packed words share, compared as the trie compares them (bit 7 dropped); the caller caps it with both lengths */
CR_DEV uint32_t crds_common(const uint8_t* a, const uint8_t* b) {
    const uint32_t* x = reinterpret_cast<const uint32_t*>(a);
    const uint32_t* y = reinterpret_cast<const uint32_t*>(b);
#pragma unroll
    for (uint32_t k = 0; k < CR_DIC_WORD_STRIDE / 4u; k++) {
        const uint32_t d = (x[k] ^ y[k]) & 0x7f7f7f7fu;
        if (d) return k * 4u + ((uint32_t)__builtin_ctz(d) >> 3);
    }
    return CR_DIC_WORD_STRIDE;
}

__global__ __launch_bounds__(CRDS_THREADS) void k_dset_sort(CrDictSetBuild P) {
    __shared__ uint32_t s_cnt[CRDS_WAVES][CRDS_BINS];      /* per wave and key: words counted, then words placed so far */
    __shared__ uint32_t s_tot[CRDS_BINS];                  /* per key: total, then where the key's run starts */
    __shared__ uint32_t s_wave[CRDS_WAVES];
    __shared__ uint32_t s_sum;
    const uint32_t tid = threadIdx.x, lane = cr_lane(), wave = cr_wave_id();
    const uint32_t w0 = P.word_off[blockIdx.x], n = P.word_off[blockIdx.x + 1u] - w0 - 1u;
    const uint8_t* words = P.words + (u64)w0 * CR_DIC_WORD_STRIDE;
    const uint8_t* wlen = P.wlen + w0;
    uint16_t* a = P.order0 + w0;
    uint16_t* b = P.order1 + w0;
    for (uint32_t i = tid; i < n; i += CRDS_THREADS) a[i] = (uint16_t)i;
    const uint32_t per = (n + CRDS_THREADS - 1u) / CRDS_THREADS * CRGPU_WAVE;      /* a wave's range, whole steps */
    const uint32_t lo = wave * per < n ? wave * per : n, hi = lo + per < n ? lo + per : n;
    __syncthreads();
    for (int col = (int)CRDS_COLS - 1; col >= 0; col--) {
        for (uint32_t i = tid; i < CRDS_WAVES * CRDS_BINS; i += CRDS_THREADS) (&s_cnt[0][0])[i] = 0u;
        __syncthreads();
        for (uint32_t i = lo + lane; i < hi; i += CRGPU_WAVE) atomicAdd(&s_cnt[wave][crds_key(words, wlen, a[i], (uint32_t)col)], 1u);
        __syncthreads();
        if (tid < CRDS_BINS) {                              /* within a key the waves' ranges follow one another */
            uint32_t run = 0;
            for (uint32_t w = 0; w < CRDS_WAVES; w++) { const uint32_t v = s_cnt[w][tid]; s_cnt[w][tid] = run; run += v; }
            s_tot[tid] = run;
        }
        __syncthreads();
        if (wave == 0) {
            uint32_t carry = 0;
            for (uint32_t r = 0; r < CRDS_BINS; r += CRGPU_WAVE) {
                const uint32_t k = r + lane, v = k < CRDS_BINS ? s_tot[k] : 0u;
                const uint32_t incl = cr_scan_incl(v);
                if (k < CRDS_BINS) s_tot[k] = carry + incl - v;
                carry += cr_lane_get(incl, 63);
            }
        }
        __syncthreads();
        for (uint32_t i0 = lo; i0 < hi; i0 += CRGPU_WAVE) {
            const uint32_t i = i0 + lane;
            const bool live = i < hi;
            const uint32_t w = live ? a[i] : 0u;
            const uint32_t key = live ? crds_key(words, wlen, w, (uint32_t)col) : 0u;
            u64 same = cr_ballot(live);                     /* the live lanes of this step that hold my key */
#pragma unroll
            for (uint32_t bit = 0; bit < 8u; bit++) {
                const bool one = (key >> bit) & 1u;
                const u64 v = cr_ballot(one);
                same &= one ? v : ~v;
            }
            const uint32_t rank = (uint32_t)__builtin_popcountll(same & ((1ull << lane) - 1ull));
            const uint32_t cnt = (uint32_t)__builtin_popcountll(same);
            uint32_t placed = 0;
            if (live) { placed = s_cnt[wave][key]; b[s_tot[key] + placed + rank] = (uint16_t)w; }
            cr_wave_sync();
            if (live && rank + 1u == cnt) s_cnt[wave][key] = placed + cnt;
            cr_wave_sync();
        }
        __syncthreads();
        uint16_t* t = a; a = b; b = t;
    }
    /* count: `a` is the sorted order */
    uint32_t running = 0;
    for (uint32_t j0 = 0; j0 < n; j0 += CRDS_THREADS) {
        const uint32_t j = j0 + tid;
        uint32_t own = 0;
        if (j < n) {
            const uint32_t w = a[j], len = wlen[w];
            uint32_t l = 0;
            if (j > 0u) {
                const uint32_t pw = a[j - 1u], plen = wlen[pw];
                l = crds_common(words + w * CR_DIC_WORD_STRIDE, words + pw * CR_DIC_WORD_STRIDE);
                l = l < len ? l : len;
                l = l < plen ? l : plen;
            }
            P.lcp[w0 + j] = (uint8_t)l;
            own = len - l;
        }
        const uint32_t incl = cr_scan_incl(own);
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        if (wave == 0) {
            const uint32_t v = lane < CRDS_WAVES ? s_wave[lane] : 0u;
            const uint32_t iv = cr_scan_incl(v);
            if (lane < CRDS_WAVES) s_wave[lane] = iv - v;
            if (lane == 63u) s_sum = iv;
        }
        __syncthreads();
        if (j < n) P.base[w0 + j] = running + s_wave[wave] + incl - own;
        running += s_sum;
        __syncthreads();
    }
    if (tid == 0) P.nnodes[blockIdx.x] = 1u + running;
}

__global__ __launch_bounds__(CRDS_THREADS) void k_dset_link(CrDictSetBuild P) {
    const uint32_t w0 = P.word_off[blockIdx.x], n = P.word_off[blockIdx.x + 1u] - w0 - 1u;
    const uint8_t* words = P.words + (u64)w0 * CR_DIC_WORD_STRIDE;
    const uint8_t* wlen = P.wlen + w0;
    const uint16_t* order = P.order1 + w0;
    uint32_t* next = P.next + P.node_off[blockIdx.x] * 128u;
    for (uint32_t depth = 0; depth < CRDS_COLS; depth++) {
        for (uint32_t j = threadIdx.x; j < n; j += CRDS_THREADS) {
            if (P.lcp[w0 + j] != depth) continue;
            const uint32_t w = order[j], len = wlen[w];
            if (len <= depth) continue;                      /* a duplicate or an empty line owns no node */
            const uint8_t* t = words + w * CR_DIC_WORD_STRIDE;
            uint32_t at = 0;                                 /* links written by other waves of the workgroup: read past the L1 */
            for (uint32_t d = 0; d < depth; d++) at = cr_ld32(&next[(u64)at * 128u + (t[d] & 127u)]);
            uint32_t node = 1u + P.base[w0 + j];
            for (uint32_t d = depth; d < len; d++) { next[(u64)at * 128u + (t[d] & 127u)] = node; at = node++; }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_dset_mark(CrDictSetBuild P) {
    const uint32_t s = blockIdx.y, w0 = P.word_off[s], n = P.word_off[s + 1u] - w0 - 1u;
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;     /* the word's number as the coder writes it: empty lines count */
    if (k >= n) return;
    const uint8_t* t = P.words + ((u64)w0 + k) * CR_DIC_WORD_STRIDE;
    const uint32_t len = P.wlen[w0 + k];
    const u64 g = P.node_off[s];
    const uint32_t* next = P.next + g * 128u;
    uint32_t at = 0;
    for (uint32_t d = 0; d < len; d++) {
        at = next[(u64)at * 128u + (t[d] & 127u)];
        atomicMin(&P.first[g + at], (int32_t)k);
    }
    atomicMax(&P.ids[g + at], (int32_t)k);                   /* (an empty line ends at the root, whose id nobody reads) */
}

__global__ __launch_bounds__(256) void k_dset_ids(CrDictSetBuild P) {
    const uint32_t s = blockIdx.y, nn = P.nnodes[s], lane = cr_lane();
    const u64 g = P.node_off[s];
    for (uint32_t row = blockIdx.x * 4u + cr_wave_id(); row < nn; row += gridDim.x * 4u) {
        const uint32_t* r = P.next + (g + row) * 128u;
        const uint32_t e0 = r[lane], e1 = r[64u + lane];
        const uint32_t f0 = e0 ? (uint32_t)P.first[g + e0] + 1u : 0u, f1 = e1 ? (uint32_t)P.first[g + e1] + 1u : 0u;
        const int32_t newest = (int32_t)cr_lane_get(cr_scan_max_incl(f0 > f1 ? f0 : f1), 63) - 1;     /* -1: no child */
        if (lane == 0u) { const int32_t last = P.ids[g + row]; P.ids[g + row] = newest > last ? -1 : last; }
    }
}

__global__ __launch_bounds__(256) void k_dset_finish(CrDictSetBuild P) {
    const uint32_t s = blockIdx.y, nn = P.nnodes[s], lane = cr_lane();
    const u64 g = P.node_off[s];
    for (uint32_t row = blockIdx.x * 4u + cr_wave_id(); row < nn; row += gridDim.x * 4u) {
        uint32_t* r = P.next + (g + row) * 128u;
        const uint32_t old0 = r[lane], old1 = r[64u + lane], space = r[' '];
        uint32_t e0 = old0, e1 = old1;
        const uint32_t hi = 64u + lane;
        if (row == 0u && hi >= 'A' && hi < 'Z') e1 = r[hi + 32u];                       /* 'Z' excluded, as the reference has it */
        if (space && !e0 && (lane == '.' || lane == ',' || lane == ':' || lane == ';')) e0 = space;
        if (e0 && P.ids[g + e0] != -1) e0 |= CR_DIC_TERMINAL;
        if (e1 && P.ids[g + e1] != -1) e1 |= CR_DIC_TERMINAL;
        if (e0 != old0) r[lane] = e0;                        /* (the stores wait for every load of the row above) */
        if (e1 != old1) r[hi] = e1;
    }
}

#endif /* CRGPU_DICTSET_TU */
#endif
