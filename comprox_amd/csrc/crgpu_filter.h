/*
 * comprox_amd/csrc/crgpu_filter.h — the `-F` pre-filters for a stream that lies in device memory
 * (crgpu_filter_blocks_dev; reference src/cr-filter.c, filter_x86_pe.c, filter_x86_elf.c, filter_bmp.c).
 *
 * The top of this file is plain C, shared by the host pass (crhost_filter.c), the plan and the kernels: the header
 * analysis of the three filters as pure functions of the bytes, the CALL/JMP operand arithmetic, the record the
 * device scan emits per image header and the two work items the plan hands back. The kernels follow for hipcc.
 *
 *   k_flt_scan<false>  tiles of 8 192 bytes of a block through LDS, the three signatures by ballots over 64-byte groups,
 *                      header analysis in the lane that hit: records per 2 048 bytes (one wave's span)
 *   k_flt_offsets      exclusive sum of those counts
 *   k_flt_scan<true>   the same walk, writing the records in stream order
 *        -- host: crf_plan_blocks walks the state machines of crhost_filter.c over the records -> work items --
 *   k_flt_e8_map       per 16 KiB tile of an E8/E9 piece: the map "operand bytes still to skip at entry -> at exit"
 *   k_flt_e8e9         entry state of the tile from the maps in front of it, of every lane by a scan under composition,
 *                      then the lane that owns an opcode converts its operand (snapshot -> stream)
 *   k_flt_watch        the 48 bytes behind an ELF image that ends inside its block: a signature there, before or after
 *                      the writes, raises the flag that sends the call to the host pass
 *   k_flt_bmp_enc      colour, left and upper deltas of one pixel from four pixels of the snapshot
 *   k_flt_bmp_rows / k_flt_bmp_colsum / k_flt_bmp_cols
 *                      decoding: sums along rows (a wave per row), sums per band of rows, then down the columns of a
 *                      band with the bands above as carry, and the colour inverse
 * No matrix instructions apply: bytes, masks and sums mod 256.
 */
#ifndef CRGPU_FILTER_H
#define CRGPU_FILTER_H

#include "../../include/crgpu.h"

#ifdef __HIPCC__
#define CRF_HD __host__ __device__ static inline
#else
#define CRF_HD static inline
#endif

enum { CRF_PE = 1, CRF_ELF = 2, CRF_BMP = 3 };

/* an image header that passed its filter's analysis with len = the rest of its block. PE: a = hdr_size, b = est;
 * ELF: a = e_shoff; BMP: a = image_off, b = width, c = height, d = bpp */
typedef struct { uint64_t pos; uint32_t kind, a, b, c, d, pad; } crf_rec;

/* CALL/JMP pass over a piece: the bytes at stream offset `off`, the loop bounds of e8e9() and the image offsets.
 * sbias: the piece's block lies in the snapshot at stream offset - sbias (the blocks are packed there back to back).
 * wg0 = first tile of the piece in the launch; watch / watch_n: candidate signature positions behind an ELF image's
 * claimed length (0 = none) */
typedef struct { uint64_t off, watch, sbias; uint32_t limit, avail; int32_t cur, end; uint32_t wg0, watch_n; } crf_e8;

/* complete rows of a BMP range: rows * row bytes at `off`. band / nbands split the decoder's column pass; wg_* = first
 * workgroup of the piece in the per-pixel, per-row and per-band launches, sums = its first cell of band sums */
typedef struct { uint64_t off, sbias; uint32_t rows, width, row, bpp, band, nbands, wg_px, wg_row, wg_band, sums; } crf_bmp;

typedef struct {
    crf_e8* e8; uint32_t n_e8, cap_e8, e8_wgs, n_watch;
    crf_bmp* bmp; uint32_t n_bmp, cap_bmp, wg_px, wg_row, wg_band, sums;
    int oom;
} crf_plan;

typedef struct { uint32_t w[24]; } crf_saved;      /* g_fs + the lossy count */

#define CRF_E8_TILE   16384u     /* bytes per workgroup of k_flt_e8_map / k_flt_e8e9 */
#define CRF_THREADS   256u

#ifdef __cplusplus
extern "C" {
#endif
/* The dispatcher and the three state machines of crhost_filter.c over the records of nb blocks instead of their bytes:
 * touched[b] = filter_inplace's return value, plan = the transforms it would have applied. Leaves the process-wide
 * filter state as filter_inplace over the same blocks leaves it. */
int  crf_plan_blocks(const crf_rec* recs, uint32_t nrec, const uint64_t* off, const uint32_t* len, uint32_t nb,
                     int en_de, uint8_t* touched, crf_plan* plan);
void crf_plan_free(crf_plan* plan);
void crf_state_save(crf_saved* s);
void crf_state_restore(const crf_saved* s);
#ifdef __cplusplus
}
#endif

CRF_HD uint32_t crf_rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
CRF_HD uint32_t crf_rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

/* "MZ", e_lfanew at 0x3c, "PE\0\0" there (filter_x86_pe.c:105-124). The reference only checks e_lfanew < len before
 * reading the signature and the headers; here every field read must lie inside the block. */
CRF_HD int crf_probe_pe(const uint8_t* buf, uint32_t len, uint32_t* hdr_size_out, uint32_t* est_out) {
    if (len < 0x40u || crf_rd16(buf) != 0x5a4du) return 0;
    const uint32_t hdr = crf_rd32(buf + 0x3c);
    if (hdr == 0 || hdr >= len || (uint64_t)hdr + 24u > len || crf_rd32(buf + hdr) != 0x00004550u) return 0;
    const uint32_t machine = crf_rd16(buf + hdr + 4), nsec = crf_rd16(buf + hdr + 6), optsz = crf_rd16(buf + hdr + 20), flags = crf_rd16(buf + hdr + 22);
    if (machine != 0x14c && (flags & 0x0002)) return 0;      /* quirk (:81): only a non-i386 EXECUTABLE image is turned away */
    const uint32_t sec_tbl = 24u + optsz;                      /* both relative to the PE signature */
    const uint32_t hdr_size = sec_tbl + nsec * 40u;
    if ((uint64_t)hdr + hdr_size > len) return 0;             /* section table inside the block */
    uint32_t est = hdr_size;
    for (uint32_t k = 0; k < nsec; k++) est += crf_rd32(buf + hdr + sec_tbl + k * 40u + 16u);   /* SizeOfRawData */
    if (est > (1u << 28)) return 0;
    *hdr_size_out = hdr_size; *est_out = est;
    return 1;
}

CRF_HD int crf_probe_elf(const uint8_t* buf, uint32_t len, uint32_t* shoff_out) {
    if (len < 52u || crf_rd32(buf) != 0x464c457fu || crf_rd16(buf + 18) != 3) return 0;      /* "\x7fELF", EM_386 */
    const uint32_t shoff = crf_rd32(buf + 32);
    if (shoff < 52u || shoff - 52u >= (1u << 30)) return 0;
    *shoff_out = shoff;
    return 1;
}

CRF_HD int crf_probe_bmp(const uint8_t* buf, uint32_t len, uint32_t* image_off, uint32_t* width_out, uint32_t* height_out, uint32_t* bpp_out) {
    if (len < 54u || crf_rd16(buf) != 0x4d42u || crf_rd16(buf + 26) != 1 || crf_rd32(buf + 30) != 0) return 0;   /* "BM", 1 plane, BI_RGB */
    const uint32_t file_size = crf_rd32(buf + 2), off = crf_rd32(buf + 10), image_size = crf_rd32(buf + 34);
    const uint32_t bpp = crf_rd16(buf + 28);
    if (image_size != 0 && off + image_size != file_size) return 0;
    if (bpp != 24 && bpp != 32) return 0;
    uint32_t width = crf_rd32(buf + 18), height = crf_rd32(buf + 22);                   /* abs() of the signed fields */
    if (width & 0x80000000u) width = 0u - width;
    if (height & 0x80000000u) height = 0u - height;
    if (width < 4 || height < 4 || width >= (1u << 20) || height >= (1u << 20)) return 0;
    *image_off = off; *width_out = width; *height_out = height; *bpp_out = bpp;
    return 1;
}

CRF_HD int crf_probe(uint32_t kind, const uint8_t* buf, uint32_t len, crf_rec* r) {
    r->kind = kind; r->a = r->b = r->c = r->d = r->pad = 0;
    if (kind == CRF_PE) return crf_probe_pe(buf, len, &r->a, &r->b);
    if (kind == CRF_ELF) return crf_probe_elf(buf, len, &r->a);
    return crf_probe_bmp(buf, len, &r->a, &r->b, &r->c, &r->d);
}

/* filter_x86opcode.h:38-62 on one operand: encoding turns a relative target that lands inside [0, end) into an
 * absolute one, decoding turns it back. `at` = image offset of the operand. */
CRF_HD int32_t crf_e8_value(int32_t v, int32_t at, int32_t end, int decode) {
    if (!decode) {
        if (v >= -at && v < end - at) v = (int32_t)((uint32_t)v + (uint32_t)at);
        else if (v > 0 && v < end) v = (int32_t)((uint32_t)v - (uint32_t)end);
    } else {
        if (v < 0) { if ((int32_t)((uint32_t)v + (uint32_t)at) >= 0) v = (int32_t)((uint32_t)v + (uint32_t)end); }
        else if (v < end) v = (int32_t)((uint32_t)v - (uint32_t)at);
    }
    return v;
}

/* e8e9()'s loop tests the byte at index i iff i < limit - 8 and i < avail, and leaves at the first opcode with
 * i + 5 > avail — a condition that then holds for every later opcode. So: the opcodes at i < crf_e8_ops are the
 * loop's candidates, nothing at or behind it is tested, and every operand read or written lies below avail. */
CRF_HD uint32_t crf_e8_ops(uint32_t limit, uint32_t avail) {
    if (limit < 8u || avail < 5u) return 0u;
    return limit - 8u < avail - 4u ? limit - 8u : avail - 4u;
}

#ifdef __HIPCC__
#include "crgpu_wave.h"
#include "crgpu_dicpick.h"                           /* cr_dic_scan1024 */

/* every kernel of this file is compiled without the packed fp32 instructions (v_pk_fma_f32, v_pk_mul_f32, v_pk_add_f32,
 * v_pk_mov_b32): some of their forms are not to be relied on on this hardware, and the compiler picks v_pk_mov_b32 for
 * plain 64-bit moves (it did in k_flt_scan<true>). Per kernel, so that no other kernel of the library is built differently. */
#ifdef __HIP_DEVICE_COMPILE__
#define CR_FLT_KERNEL __attribute__((target("no-packed-fp32-ops")))
#else
#define CR_FLT_KERNEL
#endif

#define CR_FLT_TILE    8192u                       /* bytes per workgroup of k_flt_scan */
#define CR_FLT_SPAN     (CR_FLT_TILE / 64u / (CRF_THREADS / 64u))   /* 64-byte groups per wave */
#define CR_FLT_HALO     16u                          /* bytes staged behind the tile: a signature is at most 4 */
#define CR_FLT_ID       0x4688u                      /* the identity map: state s at bits 3 s */

/* largest i < n with first[i * stride] <= t (first[0] <= t always): the block of a tile, the piece of a workgroup */
CR_DEV uint32_t cr_flt_find(const uint32_t* first, uint32_t n, uint32_t stride, uint32_t t) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (first[(size_t)mid * stride] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

struct CrFlt {
    const uint8_t*  src;
    const u64*      off;
    const uint32_t* len;
    const uint32_t* tile0;      /* nb + 1: tiles in front of block b */
    uint32_t        nb;
    uint32_t*       cnt;        /* per wave span: records, then (k_flt_offsets) records in front of it */
    uint32_t*       st;         /* [0] = records of the call, [1] = the overhang flag */
    crf_rec*        recs;
};

/* Grid = tiles, 256 threads; each wave walks CR_FLT_SPAN consecutive 64-byte groups of its tile. A group without a
 * signature costs three compares and a ballot; a lane that hits runs its filter's whole header analysis on the block's
 * bytes in memory, with len = the rest of the block. FILL = false counts, FILL = true writes at the rank. */
template <bool FILL>
CR_FLT_KERNEL __global__ __launch_bounds__(CRF_THREADS) void k_flt_scan(CrFlt F) {
    __shared__ __attribute__((aligned(16))) uint8_t s_b[CR_FLT_TILE + CR_FLT_HALO];
    const uint32_t b = cr_flt_find(F.tile0, F.nb, 1u, blockIdx.x);
    const uint32_t blen = F.len[b];
    const uint32_t t0 = (blockIdx.x - F.tile0[b]) * CR_FLT_TILE;            /* inside the block */
    const uint8_t* blk = F.src + F.off[b];
    for (uint32_t i = threadIdx.x; i < sizeof s_b / 16u; i += CRF_THREADS) {
        const uint32_t p = t0 + i * 16u;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (p + 16u <= blen) __builtin_memcpy(&v, blk + p, 16);
        else if (p < blen) {                                                  /* the block's last, partial piece */
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t k = 0; k < 16u; k++) if (p + k < blen) w[k >> 2] |= (uint32_t)blk[p + k] << (8u * (k & 3u));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(s_b + i * 16u) = v;
    }
    __syncthreads();
    const uint32_t lane = cr_lane(), wave = cr_wave_id(), span = blockIdx.x * (CRF_THREADS / 64u) + wave;
    uint32_t at = FILL ? F.cnt[span] : 0u;
    for (uint32_t g = wave * CR_FLT_SPAN; g < (wave + 1u) * CR_FLT_SPAN; g++) {
        const uint32_t i = g * 64u + lane;
        if (t0 + g * 64u >= blen) break;
        const uint32_t b0 = s_b[i], b1 = s_b[i + 1u], b2 = s_b[i + 2u], b3 = s_b[i + 3u];
        const uint32_t kind = (b0 == 'M' && b1 == 'Z') ? (uint32_t)CRF_PE : (b0 == 0x7fu && b1 == 'E' && b2 == 'L' && b3 == 'F') ? (uint32_t)CRF_ELF
                            : (b0 == 'B' && b1 == 'M') ? (uint32_t)CRF_BMP : 0u;
        if (!cr_ballot(kind != 0u)) continue;
        crf_rec r;
        bool ok = false;
        if (kind) {                                                           /* bytes behind the block read as 0: t0 + i < blen here */
            ok = crf_probe(kind, blk + t0 + i, blen - (t0 + i), &r) != 0;
            r.pos = F.off[b] + t0 + i;
        }
        const u64 acc = cr_ballot(ok);
        if (FILL && ok) F.recs[at + (uint32_t)__builtin_popcountll(acc & ((1ull << lane) - 1ull))] = r;
        at += (uint32_t)__builtin_popcountll(acc);
    }
    if (!FILL && lane == 0u) F.cnt[span] = at;
}

/* cnt: counts -> exclusive sums, st[0] = the total, st[1] = 0. One workgroup of 1024 threads. */
CR_FLT_KERNEL __global__ __launch_bounds__(CR_DIC_BLK) void k_flt_offsets(uint32_t* cnt, uint32_t n, uint32_t* st) {
    __shared__ uint32_t s_wave[CR_DIC_BLK / 64u];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += CR_DIC_BLK) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t v = t < n ? cnt[t] : 0u;
        uint32_t total;
        const uint32_t incl = cr_dic_scan1024(v, s_wave, &total);
        if (t < n) cnt[t] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0u) { st[0] = carry; st[1] = 0u; }
}

/* ---- CALL / JMP operands. State = operand bytes still to skip (0..4); a map holds the exit state for each entry
 * state at bits 3 s. ---- */

struct CrFltE8 {
    const uint8_t* snap;        /* snapshot of the blocks; a piece's stream offset x lies at snap[x - sbias] */
    uint8_t*       dst;         /* the stream */
    const crf_e8*  items;
    uint32_t       n;
    uint32_t*      tmap;        /* per tile of the launch */
    uint32_t*      st;
    int            decode;
};

/* f first, then g */
CR_DEV uint32_t cr_flt_compose(uint32_t f, uint32_t g) {
    uint32_t r = 0;
#pragma unroll
    for (uint32_t s = 0; s < 5u; s++) r |= ((g >> (3u * ((f >> (3u * s)) & 7u))) & 7u) << (3u * s);
    return r;
}

/* the lane that owns bytes [base + 64 lane, + 64) of the piece gets their mask of candidate opcodes: 64 ballots per
 * wave, each over 64 consecutive bytes (one 64-byte request) */
CR_DEV u64 cr_flt_e8_mask(const uint8_t* p, uint32_t base, uint32_t ops) {
    const uint32_t lane = cr_lane();
    u64 mine = 0;
    for (uint32_t g = 0; g < 64u; g++) {
        const uint32_t i = base + g * 64u + lane;
        if (base + g * 64u >= ops) break;
        const u64 m = cr_ballot(i < ops && (p[i] & 0xfeu) == 0xe8u);
        if (lane == g) mine = m;
    }
    return mine;
}

/* entering with s bytes to skip is state 0 with the first s bits masked off; a taken bit clears the next four */
CR_DEV uint32_t cr_flt_lane_map(u64 m) {
    uint32_t f = 0;
    if (!m) return 0u;
#pragma unroll
    for (uint32_t s = 0; s < 5u; s++) {
        uint32_t j = s;
        while (j < 64u) {
            const u64 r = m >> j;
            if (!r) { j = 64u; break; }
            j += (uint32_t)__builtin_ctzll(r) + 5u;
        }
        f |= (j - 64u) << (3u * s);
    }
    return f;
}

/* exclusive scan under composition over the 256 threads; *total = all of them. s_w: 4 words of LDS */
CR_DEV uint32_t cr_flt_scan_maps(uint32_t m, uint32_t* s_w, uint32_t* total) {
    const uint32_t lane = cr_lane(), wave = cr_wave_id();
    uint32_t incl = m;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl = cr_flt_compose(o, incl);
    }
    __syncthreads();                                                  /* s_w may still be read from the previous call */
    if (lane == 63u) s_w[wave] = incl;
    __syncthreads();
    uint32_t excl = (uint32_t)__shfl_up((int)incl, 1, 64);
    if (lane == 0u) excl = CR_FLT_ID;
    uint32_t pre = CR_FLT_ID, all = CR_FLT_ID;
    for (uint32_t k = 0; k < CRF_THREADS / 64u; k++) { if (k < wave) pre = cr_flt_compose(pre, s_w[k]); all = cr_flt_compose(all, s_w[k]); }
    *total = all;
    return cr_flt_compose(pre, excl);
}

/* Grid = tiles of all pieces. tmap[tile] = the tile's map. */
CR_FLT_KERNEL __global__ __launch_bounds__(CRF_THREADS) void k_flt_e8_map(CrFltE8 E) {
    __shared__ uint32_t s_w[CRF_THREADS / 64u];
    const crf_e8 it = E.items[cr_flt_find(&E.items[0].wg0, E.n, sizeof(crf_e8) / 4u, blockIdx.x)];
    const uint32_t ops = crf_e8_ops(it.limit, it.avail);
    const uint32_t base = (blockIdx.x - it.wg0) * CRF_E8_TILE + cr_wave_id() * 4096u;
    const u64 m = cr_flt_e8_mask(E.snap + (it.off - it.sbias), base, ops);
    uint32_t total;
    (void)cr_flt_scan_maps(cr_flt_lane_map(m), s_w, &total);
    if (threadIdx.x == 0u) E.tmap[blockIdx.x] = total;
}

/* The operand pass of e8e9(), both directions. The tile's entry state is state 0 (the piece's start) taken through the
 * maps of the tiles in front of it: every thread folds its share of them, one scan composes the shares. The lanes' maps
 * then give every lane its entry state, and the lane converts the operands of the opcodes it owns: four bytes read from
 * the snapshot, four written to the stream, wherever they lie (next lane, wave or tile; always below `avail`). */
CR_FLT_KERNEL __global__ __launch_bounds__(CRF_THREADS) void k_flt_e8e9(CrFltE8 E) {
    __shared__ uint32_t s_w[CRF_THREADS / 64u];
    const crf_e8 it = E.items[cr_flt_find(&E.items[0].wg0, E.n, sizeof(crf_e8) / 4u, blockIdx.x)];
    const uint32_t ops = crf_e8_ops(it.limit, it.avail);
    const uint32_t tile = blockIdx.x - it.wg0;
    const uint32_t share = (tile + CRF_THREADS - 1u) / CRF_THREADS;
    uint32_t f = CR_FLT_ID, total;
    for (uint32_t k = threadIdx.x * share; k < (threadIdx.x + 1u) * share && k < tile; k++) f = cr_flt_compose(f, E.tmap[it.wg0 + k]);
    (void)cr_flt_scan_maps(f, s_w, &total);
    const uint32_t tile_entry = total & 7u;
    const uint8_t* src = E.snap + (it.off - it.sbias);
    const uint32_t base = tile * CRF_E8_TILE + cr_wave_id() * 4096u;
    const u64 m = cr_flt_e8_mask(src, base, ops);
    const uint32_t excl = cr_flt_scan_maps(cr_flt_lane_map(m), s_w, &total);
    uint32_t j = (excl >> (3u * tile_entry)) & 7u;
    uint8_t* dst = E.dst + it.off;
    while (j < 64u) {
        const u64 r = m >> j;
        if (!r) break;
        j += (uint32_t)__builtin_ctzll(r);
        const uint32_t i = base + cr_lane() * 64u + j + 1u;                  /* the operand: i + 4 <= avail */
        const int32_t v = crf_e8_value((int32_t)crf_rd32(src + i), (int32_t)((uint32_t)it.cur + i), it.end, E.decode);
        dst[i] = (uint8_t)v; dst[i + 1u] = (uint8_t)((uint32_t)v >> 8); dst[i + 2u] = (uint8_t)((uint32_t)v >> 16); dst[i + 3u] = (uint8_t)((uint32_t)v >> 24);
        j += 5u;
    }
}

/* A wave per piece. An ELF image that ends inside its block is converted up to 48 bytes past the length it claims
 * (elf_step's quirk); the reference scans those bytes for headers after they were rewritten, the device scanned them
 * before. Any signature start there, in the snapshot or in the stream, raises st[1]. */
CR_FLT_KERNEL __global__ __launch_bounds__(CRF_THREADS) void k_flt_watch(CrFltE8 E) {
    const uint32_t k = blockIdx.x * (CRF_THREADS / 64u) + cr_wave_id();
    if (k >= E.n) return;
    const crf_e8 it = E.items[k];
    if (cr_lane() >= it.watch_n) return;
    const u64 p = it.watch + cr_lane();                                      /* p + 1 lies inside the block */
    const uint32_t a0 = E.snap[p - it.sbias], a1 = E.snap[p + 1u - it.sbias], b0 = E.dst[p], b1 = E.dst[p + 1u];
    const bool hit = (a0 == 'M' && a1 == 'Z') || (a0 == 0x7fu && a1 == 'E') || (a0 == 'B' && a1 == 'M') ||
                     (b0 == 'M' && b1 == 'Z') || (b0 == 0x7fu && b1 == 'E') || (b0 == 'B' && b1 == 'M');
    if (hit) cr_st32(&E.st[1], 1u);
}

/* ---- BMP. A pixel travels as one word, its px bytes at bits 8 c; sums and differences are per byte. ---- */

struct CrFltBmp {
    const uint8_t* snap;
    uint8_t*       dst;
    const crf_bmp* items;
    uint32_t       n;
    uint32_t*      sums;
};

CR_DEV uint32_t cr_flt_add8(uint32_t a, uint32_t b) { return ((a & 0x7f7f7f7fu) + (b & 0x7f7f7f7fu)) ^ ((a ^ b) & 0x80808080u); }
CR_DEV uint32_t cr_flt_sub8(uint32_t a, uint32_t b) { return ((a | 0x80808080u) - (b & 0x7f7f7f7fu)) ^ ((a ^ ~b) & 0x80808080u); }
CR_DEV uint32_t cr_flt_px_load(const uint8_t* p, uint32_t px) {
    uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    if (px == 4u) v |= (uint32_t)p[3] << 24;
    return v;
}
CR_DEV void cr_flt_px_store(uint8_t* p, uint32_t px, uint32_t v) {
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16);
    if (px == 4u) p[3] = (uint8_t)(v >> 24);
}
/* B -= G, R -= G (bytes 0 and 2 against byte 1); inverse adds */
CR_DEV uint32_t cr_flt_colour(uint32_t v, bool inverse) {
    const uint32_t g = ((v >> 8) & 0xffu) * 0x00010001u;
    return inverse ? cr_flt_add8(v, g) : cr_flt_sub8(v, g);
}

/* Encoding is position-local on the original bytes: with C = the colour transform of a pixel, the result at (y, x) is
 * C(y,x) - C(y,x-1) - C(y-1,x) + C(y-1,x-1) per byte, neighbours outside the piece's rows and the row's pixels = 0.
 * A thread per pixel; the padding behind width * px bytes of a row is never touched. */
CR_FLT_KERNEL __global__ __launch_bounds__(CRF_THREADS) void k_flt_bmp_enc(CrFltBmp B) {
    const crf_bmp it = B.items[cr_flt_find(&B.items[0].wg_px, B.n, sizeof(crf_bmp) / 4u, blockIdx.x)];
    const uint32_t t = (blockIdx.x - it.wg_px) * CRF_THREADS + threadIdx.x, px = it.bpp / 8u;
    if (t >= it.rows * it.width) return;
    const uint32_t y = t / it.width, x = t - y * it.width;
    const uint8_t* p = B.snap + (it.off - it.sbias) + (u64)y * it.row + x * px;
    uint32_t v = cr_flt_colour(cr_flt_px_load(p, px), false);
    if (x) v = cr_flt_sub8(v, cr_flt_colour(cr_flt_px_load(p - px, px), false));
    if (y) {
        uint32_t u = cr_flt_colour(cr_flt_px_load(p - it.row, px), false);
        if (x) u = cr_flt_sub8(u, cr_flt_colour(cr_flt_px_load(p - it.row - px, px), false));
        v = cr_flt_sub8(v, u);
    }
    cr_flt_px_store(B.dst + it.off + (u64)y * it.row + x * px, px, v);
}

/* Decoding, first pass: sums along a row, stride one pixel. A wave per row, 64 pixels per step, the running sum carried
 * in a register: a row of 2^20 pixels is 16 384 steps of one wave. Snapshot -> stream. */
CR_FLT_KERNEL __global__ __launch_bounds__(CRF_THREADS) void k_flt_bmp_rows(CrFltBmp B) {
    const crf_bmp it = B.items[cr_flt_find(&B.items[0].wg_row, B.n, sizeof(crf_bmp) / 4u, blockIdx.x)];
    const uint32_t y = (blockIdx.x - it.wg_row) * (CRF_THREADS / 64u) + cr_wave_id(), px = it.bpp / 8u, lane = cr_lane();
    if (y >= it.rows) return;
    const uint8_t* src = B.snap + (it.off - it.sbias) + (u64)y * it.row;
    uint8_t* dst = B.dst + it.off + (u64)y * it.row;
    uint32_t carry = 0;
    for (uint32_t x0 = 0; x0 < it.width; x0 += 64u) {
        const uint32_t x = x0 + lane;
        uint32_t incl = x < it.width ? cr_flt_px_load(src + x * px, px) : 0u;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= d) incl = cr_flt_add8(incl, o);
        }
        incl = cr_flt_add8(incl, carry);
        if (x < it.width) cr_flt_px_store(dst + x * px, px, incl);
        carry = cr_lane_get(incl, 63);
    }
}

/* second pass: the column sums of every band of `band` rows, a thread per (band, pixel column) */
CR_FLT_KERNEL __global__ __launch_bounds__(CRF_THREADS) void k_flt_bmp_colsum(CrFltBmp B) {
    const crf_bmp it = B.items[cr_flt_find(&B.items[0].wg_band, B.n, sizeof(crf_bmp) / 4u, blockIdx.x)];
    const uint32_t t = (blockIdx.x - it.wg_band) * CRF_THREADS + threadIdx.x, px = it.bpp / 8u;
    if (t >= it.nbands * it.width) return;
    const uint32_t band = t / it.width, x = t - band * it.width;
    const uint32_t y1 = (band + 1u) * it.band < it.rows ? (band + 1u) * it.band : it.rows;
    const uint8_t* p = B.dst + it.off + x * px;
    uint32_t sum = 0;
    for (uint32_t y = band * it.band; y < y1; y++) sum = cr_flt_add8(sum, cr_flt_px_load(p + (u64)y * it.row, px));
    B.sums[it.sums + t] = sum;
}

/* third pass: down the column inside the band, starting from the sums of the bands above, then the colour inverse.
 * Every thread reads and writes only its own pixels of the stream. */
CR_FLT_KERNEL __global__ __launch_bounds__(CRF_THREADS) void k_flt_bmp_cols(CrFltBmp B) {
    const crf_bmp it = B.items[cr_flt_find(&B.items[0].wg_band, B.n, sizeof(crf_bmp) / 4u, blockIdx.x)];
    const uint32_t t = (blockIdx.x - it.wg_band) * CRF_THREADS + threadIdx.x, px = it.bpp / 8u;
    if (t >= it.nbands * it.width) return;
    const uint32_t band = t / it.width, x = t - band * it.width;
    const uint32_t y1 = (band + 1u) * it.band < it.rows ? (band + 1u) * it.band : it.rows;
    uint32_t run = 0;
    for (uint32_t k = 0; k < band; k++) run = cr_flt_add8(run, B.sums[it.sums + k * it.width + x]);
    uint8_t* p = B.dst + it.off + x * px;
    for (uint32_t y = band * it.band; y < y1; y++) {
        run = cr_flt_add8(run, cr_flt_px_load(p + (u64)y * it.row, px));
        cr_flt_px_store(p + (u64)y * it.row, px, cr_flt_colour(run, true));
    }
}

#endif  /* __HIPCC__ */
#endif
