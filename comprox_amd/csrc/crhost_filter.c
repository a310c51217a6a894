/*
 * comprox_amd/csrc/crhost_filter.c — the `-F` pre-filters: the host pass (one call per datablock before the
 * dictionary stage) and the plan of the device pass (crgpu_filter_blocks_dev, crgpu_filter.h).
 *
 * Restates the behaviour of the reference's
 *   filter_inplace                 /root/reference/src/cr-filter.c:33-73   (scan, remember the filter that matched last)
 *   i386_e8e9                      src/filter_x86opcode.h:38-62           (CALL/JMP rel32 <-> absolute inside an image)
 *   pe_i386_transform              src/filter_x86_pe.c:126-159 (+ header analysis :71-124)
 *   elf_i386_transform             src/filter_x86_elf.c:127-156 (+ :102-125)
 *   bmp_transform                  src/filter_bmp.c:151-204 (+ delta passes :57-149)
 * as three small state machines behind one dispatcher. Everything that decides bytes is kept, including
 * the reference's quirks (each marked "quirk" below) — also the ELF byte counter the reference never resets,
 * which makes its transform lossy from the second ELF image of a run on: that is the DEFAULT, because the bar
 * is the reference encoder's bytes. crgpu_filter_set_mode(CRGPU_FILTER_RESTART_ELF) selects a transform that
 * restarts the counter per image and can be undone; it is not the reference's format (see elf_step). Where the reference reads or writes PAST the block
 * it was given (header fields beyond the block, an ELF code range that is 52 bytes longer than the block,
 * a code range shorter than 8 bytes) its result depends on stale heap bytes or it crashes; there this file
 * stays inside the block, and says so. The process-lifetime state of the reference (function statics) is
 * one struct here; crgpu_filter_reset() clears it (a new entry point: a library, unlike a one-shot
 * command line, filters more than one stream per process).
 *
 * What is sequential is the walk from image to image; the state machines take that walk over a `walk`, which is
 * either a block's bytes (filter_inplace: headers are analysed and ranges transformed on the spot) or the device
 * scan's records (crf_plan_blocks: a header is a record at that position, a transform is a work item). One set of
 * step functions serves both, so the state they leave is the same by construction.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/crgpu.h"
#include "crgpu_filter.h"                                  /* header analysis + operand arithmetic: shared with the device */

static void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
static uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

/* ---- CALL / JMP operands, filter_x86opcode.h:38-62 ------------------------------------------------
 * Every byte 0xE8 / 0xE9 below limit - 8 is followed by a 32-bit operand; encoding turns a relative
 * target that lands inside [0, image_end) into an absolute one, decoding turns it back. `cur` is the
 * offset of buf[0] inside the image. */
static void e8e9(uint8_t* buf, uint32_t limit, uint32_t avail, int decode, int32_t cur, int32_t end) {
    if (limit < 8u) return;                       /* the reference's unsigned `limit - 8` wraps and runs off the block */
    uint32_t i = 0;
    while (i < limit - 8u && i < avail) {         /* avail < limit only for the ELF range that overhangs its block */
        if ((buf[i++] & 0xfe) != 0xe8) continue;
        if (i + 4u > avail) break;                /* the operand is not (wholly) inside the block */
        wr32(buf + i, (uint32_t)crf_e8_value((int32_t)crf_rd32(buf + i), (int32_t)((uint32_t)cur + i), end, decode));
        i += 4;
    }
}

/* state of an image that continues into the next call (and the next datablock) */
typedef struct { int open; uint32_t cur, size; } image_state;

typedef struct {
    int last;                     /* filter_inplace's `lastproc`: 0 none, 1 PE, 2 ELF, 3 BMP */
    image_state pe, elf;
    struct { int open; int cur, size, row, bpp, width, height, skip; } bmp;
} filter_state;

static filter_state g_fs;
static int g_mode = CRGPU_FILTER_REFERENCE;
static int g_stale_elf;           /* ELF images converted with the reference's stale byte counter since the last reset */

void crgpu_filter_reset(void) { memset(&g_fs, 0, sizeof g_fs); g_stale_elf = 0; }

int crgpu_filter_lossy(void) { return g_stale_elf; }

int crgpu_filter_set_mode(int mode) {
    if (mode != CRGPU_FILTER_REFERENCE && mode != CRGPU_FILTER_RESTART_ELF) return CRGPU_E_ARG;
    g_mode = mode;
    return CRGPU_OK;
}

int crgpu_filter_mode(void) { return g_mode; }

typedef char crf_saved_fits[sizeof(filter_state) + sizeof(int) <= sizeof(crf_saved) ? 1 : -1];
void crf_state_save(crf_saved* s) { memcpy(s->w, &g_fs, sizeof g_fs); memcpy((uint8_t*)s->w + sizeof g_fs, &g_stale_elf, sizeof g_stale_elf); }
void crf_state_restore(const crf_saved* s) { memcpy(&g_fs, s->w, sizeof g_fs); memcpy(&g_stale_elf, (const uint8_t*)s->w + sizeof g_fs, sizeof g_stale_elf); }

/* ---- what the state machines walk over ---------------------------------------------------------------- */
typedef struct {
    uint8_t* buf;                 /* the block's bytes, or NULL: the plan */
    uint32_t len;
    uint64_t at;                  /* plan: stream offset of the block */
    uint64_t sbias;               /* plan: stream offset - sbias = the block's place in the snapshot (blocks packed back to back) */
    const crf_rec* recs;          /* plan: the device scan's records, ascending by position */
    uint32_t nrec;
    crf_plan* plan;
} walk;

/* first record at or behind stream offset x */
static uint32_t rec_from(const walk* w, uint64_t x) {
    uint32_t lo = 0, hi = w->nrec;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (w->recs[mid].pos < x) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

/* does filter `kind` accept a header at pos, the rest of the block being len bytes? */
static int probe(const walk* w, uint32_t kind, uint32_t pos, uint32_t len, crf_rec* h) {
    if (w->buf) return crf_probe(kind, w->buf + pos, len, h);
    const uint32_t r = rec_from(w, w->at + pos);
    if (r == w->nrec || w->recs[r].pos != w->at + pos || w->recs[r].kind != kind) return 0;
    *h = w->recs[r];
    return 1;
}

static void* plan_room(crf_plan* p, void* items, uint32_t n, uint32_t* cap, size_t each) {
    if (n < *cap) return items;
    const uint32_t want = *cap ? *cap * 2u : 64u;
    void* grown = realloc(items, (size_t)want * each);
    if (!grown) { p->oom = 1; return items; }
    *cap = want;
    return grown;
}

/* the operand pass over [pos, ...) of the block; watch_n > 0: signature positions from watch on that the pass may rewrite
 * behind the range its filter claims */
static void do_e8e9(walk* w, uint32_t pos, uint32_t limit, uint32_t avail, int decode, int32_t cur, int32_t end, uint32_t watch, uint32_t watch_n) {
    if (w->buf) { e8e9(w->buf + pos, limit, avail, decode, cur, end); return; }
    const uint32_t ops = crf_e8_ops(limit, avail);
    crf_plan* p = w->plan;
    if (!ops) return;                                       /* nothing is tested, nothing written */
    p->e8 = (crf_e8*)plan_room(p, p->e8, p->n_e8, &p->cap_e8, sizeof(crf_e8));
    if (p->n_e8 >= p->cap_e8) return;
    crf_e8* it = &p->e8[p->n_e8++];
    it->off = w->at + pos; it->sbias = w->sbias; it->limit = limit; it->avail = avail; it->cur = cur; it->end = end;
    it->watch = w->at + watch; it->watch_n = watch_n;
    it->wg0 = p->e8_wgs;
    p->e8_wgs += (ops + CRF_E8_TILE - 1u) / CRF_E8_TILE;
    if (watch_n) p->n_watch++;
}

/* ---- PE / COFF i386, filter_x86_pe.c ---------------------------------------------------------------- */
static uint32_t pe_step(walk* w, uint32_t pos, uint32_t len, int decode) {
    image_state* s = &g_fs.pe;
    uint32_t start = pos;
    uint32_t size = umin(s->size - s->cur, len), ret = size;
    if (!s->open) {
        s->cur = 0;
        crf_rec h;
        if (!probe(w, CRF_PE, pos, len, &h)) return 0;        /* crf_probe_pe: "MZ", "PE\0\0", the section table */
        const uint32_t hdr_size = h.a, est = h.b;
        /* quirk (:147-150): the code range is taken to start hdr_size bytes into the FILE — the e_lfanew
         * offset is not added — and to be est - hdr_size long */
        start = pos + hdr_size;
        s->size = est - hdr_size;
        size = umin(s->size, len - hdr_size);
        ret = size + hdr_size;
    }
    do_e8e9(w, start, size, size, decode, (int32_t)s->cur, (int32_t)s->size, 0, 0);
    s->cur += size;
    s->open = s->cur < s->size;
    return ret;
}

/* ---- ELF32 i386, filter_x86_elf.c ------------------------------------------------------------------- */
static uint32_t elf_step(walk* w, uint32_t pos, uint32_t len, int decode) {
    image_state* s = &g_fs.elf;
    uint32_t size = umin(s->size - s->cur, len), ret = size;
    if (!s->open) {
        crf_rec h;
        if (!probe(w, CRF_ELF, pos, len, &h)) return 0;       /* crf_probe_elf: "\x7fELF", EM_386, e_shoff */
        const uint32_t shoff = h.a;
        /* quirk (:143-146): the range starts behind the 52-byte header, its length is e_shoff - 52 - 52, and
         * the length is capped by len, not by len - 52. The reference's pass therefore runs up to 52 bytes
         * past the block when the image does not end inside it; here it converts every operand that lies
         * inside the block and stops there (the returned length, which positions the scan, is the reference's). */
        s->size = shoff - 52u - 52u;
        /* quirk (:131-134, function-scope statics): the reference never resets its ELF byte counter (`curr`), so a
         * second ELF image in one run is converted with the first image's length as its start offset — and is
         * taken to be complete as soon as that stale counter passes its length. With offset > length the two
         * operand ranges of i386_e8e9 overlap and the transform cannot be undone (tests/golden/golden_filter.json,
         * cases two_elf / tar_like: the reference's own FILTER_DEC does not restore them). Kept by default: the
         * encoder's bytes are the reference's. CRGPU_FILTER_RESTART_ELF restarts the counter with every image —
         * a transform that round-trips, marked m_filt = 2 in the files of comp*-gpu -FF. */
        if (g_mode == CRGPU_FILTER_RESTART_ELF) s->cur = 0;
        else if (s->cur != 0) g_stale_elf++;     /* the caller can see it (crgpu_filter_lossy): comp*-gpu -F warns */
        size = umin(s->size, len);
        ret = size;
        /* an image that ends inside the block: operands up to byte size + 48 are rewritten, bytes the scan has yet to
         * look at. The device pass watches the signature positions there (both bytes inside the block). */
        const uint32_t watch_n = size < len ? umin(size + 48u, len - 1u) - size : 0u;
        do_e8e9(w, pos + 52u, size, len - 52u, decode, (int32_t)s->cur, (int32_t)s->size, pos + size, watch_n);
    } else {
        do_e8e9(w, pos, size, size, decode, (int32_t)s->cur, (int32_t)s->size, 0, 0);
    }
    s->cur += size;
    s->open = s->cur < s->size;
    return ret;
}

/* ---- BMP 24 / 32 bpp, filter_bmp.c ------------------------------------------------------------------- */
/* colour (B -= G, R -= G), then left-neighbour and upper-neighbour deltas over the complete rows of the
 * range; decoding undoes them in the opposite order (:57-149) */
static uint32_t bmp_rows(uint8_t* buf, uint32_t len, int width, int row, int bpp, int decode) {
    const int rows = (int)(len / (uint32_t)row), px = bpp / 8;
    if (!decode) {
        for (int y = 0; y < rows; y++) {
            uint8_t* r = buf + (size_t)y * row;
            for (int x = 0; x < width; x++) { r[x * px + 0] -= r[x * px + 1]; r[x * px + 2] -= r[x * px + 1]; }
        }
        for (int y = 0; y < rows; y++) {
            uint8_t* r = buf + (size_t)y * row;
            for (int x = width - 1; x > 0; x--) for (int c = 0; c < px; c++) r[x * px + c] -= r[(x - 1) * px + c];
        }
        for (int y = rows - 1; y > 0; y--) {
            uint8_t *r = buf + (size_t)y * row, *u = r - row;
            for (int x = 0; x < width * px; x++) r[x] -= u[x];
        }
    } else {
        for (int y = 0; y < rows; y++) {
            uint8_t* r = buf + (size_t)y * row;
            for (int x = 1; x < width; x++) for (int c = 0; c < px; c++) r[x * px + c] += r[(x - 1) * px + c];
        }
        for (int y = 1; y < rows; y++) {
            uint8_t *r = buf + (size_t)y * row, *u = r - row;
            for (int x = 0; x < width * px; x++) r[x] += u[x];
        }
        for (int y = 0; y < rows; y++) {
            uint8_t* r = buf + (size_t)y * row;
            for (int x = 0; x < width; x++) { r[x * px + 0] += r[x * px + 1]; r[x * px + 2] += r[x * px + 1]; }
        }
    }
    return (uint32_t)row * (uint32_t)rows;
}

/* the complete rows of [pos, pos + len); returns their bytes */
static uint32_t do_bmp_rows(walk* w, uint32_t pos, uint32_t len, int width, int row, int bpp, int decode) {
    if (w->buf) return bmp_rows(w->buf + pos, len, width, row, bpp, decode);
    const uint32_t rows = len / (uint32_t)row;
    crf_plan* p = w->plan;
    if (!rows) return 0;
    p->bmp = (crf_bmp*)plan_room(p, p->bmp, p->n_bmp, &p->cap_bmp, sizeof(crf_bmp));
    if (p->n_bmp >= p->cap_bmp) return (uint32_t)row * rows;
    crf_bmp* it = &p->bmp[p->n_bmp++];
    it->off = w->at + pos; it->sbias = w->sbias; it->rows = rows; it->width = (uint32_t)width; it->row = (uint32_t)row; it->bpp = (uint32_t)bpp;
    /* the decoder's column pass: bands of about sqrt(rows) rows, so that a band's walk and the carry over the bands
     * above it are equally long and a tall, narrow piece still spreads over rows / band x width threads */
    it->band = 16u;
    while (it->band * it->band < rows) it->band++;
    it->nbands = (rows + it->band - 1u) / it->band;
    it->wg_px = p->wg_px; it->wg_row = p->wg_row; it->wg_band = p->wg_band; it->sums = p->sums;
    p->wg_px += (rows * it->width + CRF_THREADS - 1u) / CRF_THREADS;
    p->wg_row += (rows + CRF_THREADS / 64u - 1u) / (CRF_THREADS / 64u);
    p->wg_band += (it->nbands * it->width + CRF_THREADS - 1u) / CRF_THREADS;
    p->sums += it->nbands * it->width;
    return (uint32_t)row * rows;
}

static uint32_t bmp_step(walk* w, uint32_t pos, uint32_t len, int decode) {
    if (!g_fs.bmp.open) {
        crf_rec h;
        if (!probe(w, CRF_BMP, pos, len, &h)) return 0;       /* crf_probe_bmp: "BM", 1 plane, BI_RGB, 24 / 32 bpp, 4 <= w, h < 2^20 */
        const uint32_t image_off = h.a;
        const int width = (int)h.b, height = (int)h.c, bpp = (int)h.d;
        g_fs.bmp.width = width; g_fs.bmp.height = height; g_fs.bmp.bpp = bpp;
        g_fs.bmp.row = (bpp * width + 31) / 32 * 4;
        /* quirk (:183-188): the header is skipped in one step and the byte counter starts at the pixel
         * offset, not at 0, so the last image_off bytes of the pixel array are left alone */
        g_fs.bmp.cur = (int)image_off;
        g_fs.bmp.size = height * g_fs.bmp.row;
        g_fs.bmp.skip = 0;
        g_fs.bmp.open = 1;
        return image_off;
    }
    if (g_fs.bmp.skip > 0) {                                   /* the row that straddled the previous range (:190-195) */
        const uint32_t n = umin((uint32_t)g_fs.bmp.skip, len);
        g_fs.bmp.cur += (int)n;
        g_fs.bmp.skip -= (int)n;
        return n;
    }
    const uint32_t done = do_bmp_rows(w, pos, umin(len, (uint32_t)(g_fs.bmp.size - g_fs.bmp.cur)), g_fs.bmp.width, g_fs.bmp.row, g_fs.bmp.bpp, decode);
    g_fs.bmp.cur += (int)done;
    if (g_fs.bmp.cur < g_fs.bmp.size) g_fs.bmp.skip = (int)umin((uint32_t)g_fs.bmp.row, (uint32_t)(g_fs.bmp.size - g_fs.bmp.cur));
    else g_fs.bmp.open = 0;
    return done;
}

/* ---- dispatcher, cr-filter.c:33-73 -------------------------------------------------------------------- */
static uint32_t run(walk* w, int which, uint32_t pos, uint32_t len, int decode) {
    return which == 1 ? pe_step(w, pos, len, decode) : which == 2 ? elf_step(w, pos, len, decode) : bmp_step(w, pos, len, decode);
}

/* Try the filter that matched last, then PE, ELF, BMP, at every position a filter has not claimed.
 * Returns 1 when any filter touched the block (the block header's m_filt, src/main.c:183-185,200). */
static int walk_block(walk* w, int decode) {
    int touched = 0;
    const uint32_t len = w->len;
    for (uint32_t pos = 0; pos < len; pos++) {
        if (g_fs.last) {
            const uint32_t n = run(w, g_fs.last, pos, len - pos, decode);
            if (n == 0) g_fs.last = 0;
            else { touched = 1; pos += n - 1u; continue; }
        }
        if (!w->buf && !g_fs.pe.open && !g_fs.elf.open && !g_fs.bmp.open) {
            /* the plan: with no image open, a position without a record fails all three filters and changes nothing
             * (`last` is 0 here) — go to the next record of this block */
            const uint32_t r = rec_from(w, w->at + pos);
            if (r == w->nrec || w->recs[r].pos >= w->at + len) break;
            pos = (uint32_t)(w->recs[r].pos - w->at);
        }
        for (int k = 1; k <= 3; k++) {
            const uint32_t n = run(w, k, pos, len - pos, decode);
            if (n > 0) { touched = 1; g_fs.last = k; pos += n - 1u; break; }
        }
    }
    return touched;
}

int filter_inplace(unsigned char* buf, uint32_t len, int en_de) {
    walk w;
    memset(&w, 0, sizeof w);
    w.buf = buf; w.len = len;
    return walk_block(&w, en_de != 0);
}

int crf_plan_blocks(const crf_rec* recs, uint32_t nrec, const uint64_t* off, const uint32_t* len, uint32_t nb,
                    int en_de, uint8_t* touched, crf_plan* plan) {
    memset(plan, 0, sizeof *plan);
    uint64_t packed = 0;
    for (uint32_t b = 0; b < nb; b++) {
        walk w;
        memset(&w, 0, sizeof w);
        w.len = len[b]; w.at = off[b]; w.sbias = off[b] - packed;
        packed += len[b]; w.recs = recs; w.nrec = nrec; w.plan = plan;
        touched[b] = (uint8_t)walk_block(&w, en_de != 0);
    }
    return plan->oom ? CRGPU_E_NOMEM : CRGPU_OK;
}

void crf_plan_free(crf_plan* plan) {
    free(plan->e8); free(plan->bmp);
    memset(plan, 0, sizeof *plan);
}
