/*
 * include/crgpu.h — C-ABI of libcrgpu.so, the MI355X (gfx950) block codec behind comprox's
 * data_block_t entry points.
 *
 * Drop-in boundary. Every symbol below is plain C (pointers and sizes, no C++
 * or torch types) and names the reference interface it stands in for:
 *
 *   data_block_t, data_block_*    /root/reference/src/cr-datablock.h:35-46, cr-datablock.c:31-56
 *   reset_models/lzencode/lzdecode /root/reference/src/main.c:55-59 (extern decls the block loop
 *                                  links against), bodies in src/ropmain/cr-coder.c:73-83,119-292
 *                                  (comprop) and src/roxmain/cr-coder.c:88-114,153-318,390-526
 *   crgpu_*_blocks*               the batched form of the block loop src/main.c:174-206 (encode)
 *                                  and src/main.c:263-292 (decode) run with reset_models() before
 *                                  every block, i.e. independent datablocks
 *
 * The codec work happens in hand-written HIP kernels (comprox_amd/csrc/crgpu.hip + crgpu_*.h); there
 * is no CPU fallback: every entry point returns CRGPU_E_NODEVICE when no gfx950 device is usable.
 */
#ifndef CRGPU_H
#define CRGPU_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (the reference's entry points are void; the batched API reports) ---- */
#define CRGPU_OK            0
#define CRGPU_E_NODEVICE   -1   /* no HIP device / wrong architecture / HIP runtime error       */
#define CRGPU_E_ARG        -2   /* NULL pointer, bad codec id, block larger than CRGPU_MAX_BLOCK */
#define CRGPU_E_NOMEM      -3   /* device or host allocation failed                             */
#define CRGPU_E_CORRUPT    -4   /* decode: a block header is inconsistent with its capacity     */

/* ---- codecs: which reference binary's lzencode/lzdecode is mirrored ---- */
#define CRGPU_CODEC_ROP     1   /* comprop: LZP + one PPM/range stream (src/ropmain/)           */
#define CRGPU_CODEC_ROX     2   /* comprox: LZ77 + PPM + three side streams (src/roxmain/)      */
#define CRGPU_CODEC_ROLZ    3   /* comprolz: ROLZ + PPM + one side stream (src/rolzmain/)       */

#define CRGPU_ROP_HEADER   20u  /* sizeof(block_header), src/ropmain/cr-coder.c:59-66           */
#define CRGPU_ROX_HEADER   32u  /* sizeof(block_header), src/roxmain/cr-coder.c:69-81           */
#define CRGPU_ROLZ_HEADER  16u  /* sizeof(block_header), src/rolzmain/cr-coder.c:63-71          */
#define CRGPU_MAX_BLOCK    (16u << 20)  /* largest datablock (reference default -b16, src/main.c:62). The
                                           codec stage accepts CRGPU_MAX_BLOCK + 1 bytes: dictionary_encode hands
                                           a block it could not shrink on as raw copy + flag byte
                                           (src/cr-diccode.c:208-217)                                        */

/* Worst-case encoded size of an n-byte block for `codec` (stored form: header + raw bytes). */
uint32_t crgpu_bound(int codec, uint32_t n);

/* ---- context: one per (process, GPU); owns the stream and the per-workgroup model arena ---- */
typedef struct crgpu_ctx crgpu_ctx;

int  crgpu_create(crgpu_ctx** out, int device);
void crgpu_destroy(crgpu_ctx* ctx);
const char* crgpu_last_error(const crgpu_ctx* ctx);   /* text of the last HIP failure, or ""   */
/* comprox codec: chain nodes examined per match search — the reference's -m switch
 * (match_limit, src/roxmain/cr-matcher.c:39, default 40). */
int  crgpu_rox_set_chain_limit(crgpu_ctx* ctx, uint32_t limit);
/* flexible_parsing (`-f`, src/roxmain/cr-matcher.c:32,253-289 and src/rolzmain/cr-matcher.c:30,143-167): the
 * parser of comprox / comprolz cuts a match where "this match + what follows it" prices best. Off by default. */
int  crgpu_set_flexible_parsing(crgpu_ctx* ctx, int on);
/* Route work to a caller-owned hipStream_t (NULL = the context's own stream). */
int  crgpu_set_stream(crgpu_ctx* ctx, void* hip_stream);
/* Diagnostic switches (the defaults are the product). crgpu_create reads the environment variable of the same
 * name ONCE; nothing on the call path looks at the environment. */
#define CRGPU_OPT_WG_PER_CU        1   /* resident workgroups per CU, 1..32 (default 16); each owns one model arena     */
#define CRGPU_OPT_ONE_WAVE_ENCODER 2   /* 1: the model-carrying one-wave coders (k_rop_encode / k_rox_encode /
                                          k_rolz_encode, what the shims run) instead of the kernel pipeline            */
#define CRGPU_OPT_ONE_WAVE_DECODER 3   /* 1: the model-carrying C++ decoders (k_rop_decode / k_rox_decode /
                                          k_rolz_decode) instead of the assembly step                                  */
#define CRGPU_OPT_LZP_GRID         4   /* at most this many workgroups for k_rop_lzp (0 = no limit)                    */
#define CRGPU_OPT_MATCH_GRID       5   /* the same for k_rox_match / k_rolz_match                                      */
#define CRGPU_OPT_LZP_TABLES       6   /* 1: the older kernels — every block through the table sweeps (k_rop_lzp, k_rop_links,
                                          the sweeps inside k_rox_match / k_rolz_match) instead of the sorts in LDS, and
                                          k_rop_o2 / k_rop_o3 walking their chains by tickets instead of slot ranges. Same
                                          bytes either way: the parity tests run both                                   */
#define CRGPU_OPT_STAGE_LOG        7   /* 1: keep the HIP-event boundaries of every kernel of every call until
                                          crgpu_stage_log_read folds them up (a timed loop then needs no event wait
                                          between its calls); 0: off, log dropped                                      */
#define CRGPU_OPT_DECODER_HELPER    8   /* 1: comprop's batched decoder as k_rop_decode_v5h — a workgroup of two waves per block, the
                                          second one preparing the escape step's order-1 sums (cr-ppm.c:209-211) from what the
                                          coder wave posts in LDS. Same bytes; measured slower than the one-wave kernel
                                          (DESIGN.md), kept for the parity tests and the record                              */
#define CRGPU_OPT_DECODER_LDS_NODES  9   /* 1 (default): comprop's batched decoder keeps its first dense order-2 nodes in LDS as well
                                          (k_rop_decode_v5, 8.7 KB of LDS per block in flight); 0: k_rop_decode_v5s, 272 bytes — for a
                                          caller that runs another context's encode calls beside this one's decodes, so that the
                                          decoder's workgroups leave room on a CU for a sorting kernel's 152 KB. Same bytes          */
#define CRGPU_OPT_DICPICK_EPOCHS    10   /* crgpu_dicpick_dev: purges of the reference's word map replayed on the device before the
                                          stream goes to the host census instead (default 256; 0: always the host census)  */
#define CRGPU_OPT_SEQDEC_GRID       11   /* at most this many workgroups for the k_seqdec kernels (0 = no limit): with fewer than there are
                                          sequences a wave takes a second sequence from the ticket in the same launch       */
int  crgpu_set_option(crgpu_ctx* ctx, int option, int value);

/*
 * Batched independent-datablock codec, DEVICE pointers (inputs already resident in HBM).
 * Block b reads  in[in_off[b] .. in_off[b]+in_size[b])  and writes its result at
 * out[out_off[b] ..], storing the produced byte count in out_size[b].
 *   encode: out must hold crgpu_bound(codec, in_size[b]) bytes per block.
 *   decode: out_cap[b] is the room at out_off[b]; a block that would overflow it, or whose
 *           header is malformed, yields out_size[b] = 0xFFFFFFFF and the call returns
 *           CRGPU_E_CORRUPT after all other blocks have been decoded.
 * Each block is coded with freshly reset models (reset_models() semantics).
 * All arrays (in_off, in_size, out_off, out_cap, out_size) are device arrays of nblocks entries.
 * The call enqueues on the context's stream and returns without synchronising unless
 * `sync` is non-zero.
 */
int crgpu_encode_blocks_dev(crgpu_ctx* ctx, int codec,
                            const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                            uint32_t nblocks, uint32_t max_block,
                            uint8_t* out, const uint64_t* out_off, uint32_t* out_size, int sync);
int crgpu_decode_blocks_dev(crgpu_ctx* ctx, int codec,
                            const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                            uint32_t nblocks, uint32_t max_block,
                            uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                            uint32_t* out_size, int sync);

/* comprop with models that outlive the block: the reference's ppm_model_t (src/cr-ppm.h:36-41) survives from one lzencode to
 * the next until reset_models(), and the stock container codes every file larger than one block that way. A crgpu_models
 * holds that state in device memory (26 280 192 bytes, and as much again for the copy the abort point goes back to),
 * indexed by the reference's own keys; create leaves it in the ppm_model_init state, reset puts it back there (enqueued on
 * the context's stream). It belongs to the context it was created on. */
typedef struct crgpu_models crgpu_models;
int  crgpu_models_create(crgpu_ctx* ctx, crgpu_models** out);
void crgpu_models_destroy(crgpu_models* m);
int  crgpu_models_reset(crgpu_ctx* ctx, crgpu_models* m);
/* Pointer conventions of crgpu_encode_blocks_dev. Block 0 starts from the state in `m`, block i continues block i - 1, and on
 * return `m` holds the state behind the last block — a block that ends stored leaves it where lzencode gave up
 * (src/ropmain/cr-coder.c:204-206), one under 16 bytes does not touch it. Every block's bytes are what the reference's lzencode
 * writes for it in that sequence. codec must be CRGPU_CODEC_ROP (CRGPU_E_ARG otherwise: comprox and comprolz carry side models
 * too). The call returns when the blocks are coded. */
int crgpu_encode_blocks_carried_dev(crgpu_ctx* ctx, int codec, crgpu_models* m,
                                    const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size, uint32_t nblocks,
                                    uint8_t* out, const uint64_t* out_off, uint32_t* out_size);
/* ... and with HOST pointers (the conventions of crgpu_encode_blocks) */
int crgpu_encode_blocks_carried(crgpu_ctx* ctx, int codec, crgpu_models* m,
                                const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size, uint32_t nblocks,
                                uint8_t* out, const uint64_t* out_off, uint32_t* out_size);

/* Many sequences of dependent comprop blocks in one call (an archive's members, a directory, a request queue): step t of the
 * call codes block t of every sequence that has one, in one pass of the kernel pipeline. A crgpu_model_set holds `nseq` model
 * stores (slots, 26 280 192 bytes each) for blocks of up to `max_block` bytes, and per slot an undo log of
 *   65 792 + 280 x min(E, 65 536) + 8 x min(E, 1 << 22) bytes, E = align_up(max(max_block, 1024) + max_block / 64 + 128, 64)
 * — the chain start states a block overwrites, which a block that ends stored goes back to: no second store per sequence
 * and no store-sized copy per block. create leaves every slot in the ppm_model_init state; reset puts the slots
 * which[0 .. n) back there (which == NULL: all of them; `which` is HOST memory). The set belongs to its context.
 *
 * A set is made for ONE codec and the calls on it must name that codec. comprox and comprolz keep, beside the PPM model, the
 * small adaptive models of their side streams between blocks (roxmain/cr-coder.c:55-60: len_model, pos_models[6],
 * spos_model; rolzmain: len_model, idx_model). A set of theirs holds per slot the same 26 280 192-byte store and undo log and,
 * in an allocation of its own, 2 x 4 352 = 8 704 bytes more: the side models (u16[8][256] counts and their totals) and the
 * snapshot of them from in front of the slot's current block, which a block that ends stored goes back to. reset puts them
 * back to reset_models' state too. Per-block scratch is one slot per sequence, reused every step: 16 x (max(max_block, 1024)
 * + 64) bytes of match tables (comprolz: ring and link tables) and 3 x (2 x max_block + 256) bytes of side-stream staging,
 * both rounded up to 1 KiB / 256 bytes. crgpu_model_set_create is crgpu_model_set_create_codec with CRGPU_CODEC_ROP. */
typedef struct crgpu_model_set crgpu_model_set;
int  crgpu_model_set_create(crgpu_ctx* ctx, uint32_t nseq, uint32_t max_block, crgpu_model_set** out);
int  crgpu_model_set_create_codec(crgpu_ctx* ctx, int codec, uint32_t nseq, uint32_t max_block, crgpu_model_set** out);
void crgpu_model_set_destroy(crgpu_model_set* set);
int  crgpu_model_set_reset(crgpu_ctx* ctx, crgpu_model_set* set, const uint32_t* which, uint32_t n);
/* Pointer conventions of crgpu_encode_blocks_dev, except seq_first: HOST memory, nseq + 1 entries, ascending. Sequence s owns
 * the blocks seq_first[s] .. seq_first[s + 1] - 1 of the flat block arrays (it may own none) and slot s of the set: its first
 * block starts from the slot's state, block i continues block i - 1, and on return the slot holds the state behind the
 * sequence's last block — so a sequence may be fed in slices over several calls; a slot without a block in a call is not
 * touched. Every block's bytes are what the reference's lzencode writes for it in its sequence; the rules of
 * crgpu_encode_blocks_carried_dev for blocks under 16 bytes and blocks that end stored hold per sequence (comprop). A comprox
 * or comprolz block ends stored when the header (32 / 16 bytes) and the main stream reach the input's size behind any token;
 * the models then stay as they stood behind that token, side models included, and no block is too small to move them: one
 * of up to header bytes is given up at its first token (a comprolz block of 1 byte has no token and comes out coded, one of
 * 0 bytes leaves its slot alone). CRGPU_E_ARG for a codec other than the set's, a one-wave context, a block above the set's max_block, more sequences than slots, a
 * descending seq_first and a set of another context. The call returns when all blocks are coded. */
int crgpu_encode_sequences_carried_dev(crgpu_ctx* ctx, int codec, crgpu_model_set* set,
                                       const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                                       const uint32_t* seq_first, uint32_t nseq,
                                       uint8_t* out, const uint64_t* out_off, uint32_t* out_size);
/* ... and with HOST pointers (the conventions of crgpu_encode_blocks) */
int crgpu_encode_sequences_carried(crgpu_ctx* ctx, int codec, crgpu_model_set* set,
                                   const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                                   const uint32_t* seq_first, uint32_t nseq,
                                   uint8_t* out, const uint64_t* out_off, uint32_t* out_size);

/* ... and back: many sequences of dependent comprop blocks DECODED in one kernel launch. One wavefront takes a sequence and
 * walks its blocks front to back, so S sequences decode side by side where the lzdecode shim decodes one block per call. A
 * crgpu_decode_set holds `nseq` slots in one allocation; a slot is a decoder model in the batched decoder's own format —
 * directory words, 65 536 node lines of 128 bytes, order-1 rows, the direct order-3 table u16[1 << 22], a dense area of
 * 65 536 slots of 256 bytes (one per 16-bit context: a sequence of any length cannot run out) — and, PER SLOT, the LZP tables
 * for blocks of up to `max_block` bytes, emptied in front of every block as matcher_init does. Bytes per slot:
 *   34 144 256 + 16 x C,  C = the power of two at or above 2 x max(1024, max_block rounded up to 1 KiB), at most 1 << 26
 * (36 241 408 for 64 KiB blocks). create leaves every slot in the ppm_model_init state; reset puts the slots which[0 .. n)
 * back there (which == NULL: all of them; `which` is HOST memory) by marking them — the kernel that next picks a marked slot
 * up does the work. CRGPU_E_ARG for no slot or more than 65 535, and for a max_block the decoder's layout cannot address
 * (above CRGPU_MAX_BLOCK + 1); CRGPU_E_NOMEM when the allocation fails. The set belongs to its context. */
typedef struct crgpu_decode_set crgpu_decode_set;
int  crgpu_decode_set_create(crgpu_ctx* ctx, uint32_t nseq, uint32_t max_block, crgpu_decode_set** out);
/* The same for any of the three codecs (crgpu_decode_set_create is this with CRGPU_CODEC_ROP); the set remembers its codec and
 * serves calls that name it. A comprox / comprolz slot holds the same model tables and, in place of the LZP tables, an 8 KiB
 * keep area for the side models (eight / two adaptive models of 256 symbols, parked there between calls) with its staging
 * room; a comprolz slot also holds that codec's matcher — link tables, ring history (blocks up to 1 MiB), ring heads — emptied
 * in front of every block as matcher_init does. Bytes per slot, M = max(1024, max_block rounded up to 1 KiB):
 *   comprox   33 890 304 + 3 x (2 M + 256), rounded up to 4 KiB                      (34 287 616 for 64 KiB blocks)
 *   comprolz  the same + 12 M + 32 M (M <= 1 MiB only) + 1 048 576                   (38 219 776 for 64 KiB blocks)
 * CRGPU_E_ARG also for a codec that is none of the three. */
int  crgpu_decode_set_create_codec(crgpu_ctx* ctx, int codec, uint32_t nseq, uint32_t max_block, crgpu_decode_set** out);
void crgpu_decode_set_destroy(crgpu_decode_set* set);
int  crgpu_decode_set_reset(crgpu_ctx* ctx, crgpu_decode_set* set, const uint32_t* which, uint32_t n);
/* diagnostic: the order-2 nodes of a slot that have outgrown their line and live in its dense area; waits for the stream */
int  crgpu_decode_set_dense_nodes(crgpu_ctx* ctx, crgpu_decode_set* set, uint32_t slot, uint32_t* count);
/* Pointer conventions of crgpu_decode_blocks_dev, except seq_first: HOST memory, nseq + 1 entries, ascending. Sequence s owns
 * the blocks seq_first[s] .. seq_first[s + 1] - 1 and slot s: block 0 starts from the slot's state, block i continues block
 * i - 1, and on return the slot holds the state behind the sequence's last block — so a sequence may be fed in slices over
 * several calls; a slot without a block in a call is not touched. Every block's output is what the reference's lzdecode
 * produces for it in that sequence; a stored block is copied out and leaves the models and the context register alone.
 * A block fails — out_size = 0xFFFFFFFF — on a header shorter than 20 bytes, an original size above out_cap or above the
 * set's max_block, or a damaged stream; every later block of its slot then reports 0xFFFFFFFF undecoded, in this call and in
 * later ones, until the slot is reset. CRGPU_E_ARG for a codec other than the set's, more sequences than slots, a
 * descending seq_first, a set of another context and a block whose in_size exceeds crgpu_bound(the set's codec, max_block).
 * The block sizes are read back once in front of the launch (that check and the order of the sequences need them); the
 * decode itself is one launch that the call only enqueues unless `sync` is non-zero, in which case it returns
 * CRGPU_E_CORRUPT if a block failed, after every other sequence has been decoded. */
int crgpu_decode_sequences_carried_dev(crgpu_ctx* ctx, int codec, crgpu_decode_set* set,
                                       const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                                       const uint32_t* seq_first, uint32_t nseq,
                                       uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_size, int sync);
/* ... and with HOST pointers (the conventions of crgpu_decode_blocks; CRGPU_E_CORRUPT as there) */
int crgpu_decode_sequences_carried(crgpu_ctx* ctx, int codec, crgpu_decode_set* set,
                                   const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                                   const uint32_t* seq_first, uint32_t nseq,
                                   uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_size);

/* Device-side concatenation of a batch (`k_pack`; the write loop of src/main.c:198-205 as one contiguous run):
 * payload b = in[in_off[b] .. +in_size[b]) is copied to out[out_off[b] ..) where out_off is the exclusive sum of the
 * slots in front of it. with_headers != 0: every non-empty block is preceded by the container's packed
 * {u32 m_size, u8 m_filt, u8 m_prec} header (src/main.c:90-94; m_filt from filt[b] or 0, m_prec = prec) and empty
 * blocks are skipped, as `if(yb->m_size > 0)` does; out_off[b] is the PAYLOAD's position. total[0] = bytes laid out,
 * total[1] = blocks whose size is 0xFFFFFFFF (failed; skipped). All pointers are device pointers; out needs
 * sum(in_size) + 6 * nblocks bytes at most. */
int crgpu_pack_blocks_dev(crgpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                          uint32_t nblocks, const uint8_t* filt, int prec, int with_headers,
                          uint8_t* out, uint64_t* out_off, uint64_t* total, int sync);

/* The scan alone: out_off[b] = sum of sizes[k] for k < b, total[0] = the sum, total[1] = entries equal to 0xFFFFFFFF
 * (counted as 0). */
int crgpu_offsets_dev(crgpu_ctx* ctx, const uint32_t* sizes, uint32_t nblocks, uint64_t* out_off, uint64_t* total, int sync);

/* Same contract with HOST pointers: stages through device buffers (H2D, kernels, D2H). */
int crgpu_encode_blocks(crgpu_ctx* ctx, int codec,
                        const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                        uint32_t nblocks, uint8_t* out, const uint64_t* out_off, uint32_t* out_size);
int crgpu_decode_blocks(crgpu_ctx* ctx, int codec,
                        const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                        uint32_t nblocks, uint8_t* out, const uint64_t* out_off,
                        const uint32_t* out_cap, uint32_t* out_size);

/* Timing of the most recent *_dev / host call on this context, from HIP events recorded on the
 * stream the kernels ran on: milliseconds spent in the dominant codec kernel. */
float crgpu_last_kernel_ms(const crgpu_ctx* ctx);
/* An encode call runs a matching pre-pass (k_rop_lzp / k_rox_match) and then the coding kernels;
 * crgpu_last_kernel_ms covers all of them, this returns the share of the pre-pass (-1 after a decode call). */
float crgpu_last_lzp_ms(const crgpu_ctx* ctx);
/* Every kernel of the most recent call, in launch order: names[i] (static strings) and ms[i] for
 * i < min(room, return value). Returns the number of kernels the call launched, -1 on error. */
int crgpu_last_stage_ms(const crgpu_ctx* ctx, const char** names, float* ms, int room);

/* With CRGPU_OPT_STAGE_LOG on: for every kernel name launched since the log was switched on or last read, the summed
 * milliseconds (HIP events on the kernels' stream) and the number of launches; waits for the stream once and empties
 * the log (also when it fails). names / total_ms / launches have `room` entries; returns the number of distinct kernels
 * — a value above `room` means that many were seen and only the first `room` stored — or -1 on error. */
int crgpu_stage_log_read(crgpu_ctx* ctx, const char** names, float* total_ms, uint32_t* launches, int room);

/* Which match pre-pass took the blocks of the most recent encode call on this context: counts[0] = the table sweep in HBM
 * (k_rop_lzp / k_rox_match / k_rolz_match), counts[1] = the LDS sort for blocks of up to 28 672 bytes, counts[2] = the LDS sort
 * in groups by key for blocks of up to 65 537 bytes (a block whose keys do not split falls back to the sweep). They stand
 * for the reference's dense "last position with this key" tables (src/ropmain/cr-matcher.c:35-50 and siblings). */
int crgpu_last_prepass_paths(crgpu_ctx* ctx, uint32_t counts[3]);

/* ---- static-dictionary stage (reference: src/cr-diccode.c) ------------------------------------
 * crgpu_dict_create   == dictionary_load(text, 1) (src/cr-diccode.c:76-118): parses the dictionary
 *                        text produced by dicpick() (one word per line, NUL-terminated), builds the
 *                        reference's trie on the host and uploads it. One dictionary per file.
 * crgpu_dict_*_blocks == dictionary_encode (src/cr-diccode.c:142-221) / dictionary_decode
 *                        (:223-283) per datablock. encode: out must hold in_size[b] + 1 bytes per block
 *                        (raw copy + flag byte when substitution does not shrink the block);
 *                        decode: as crgpu_decode_blocks (out_cap, 0xFFFFFFFF on malformed input). */
typedef struct crgpu_dict crgpu_dict;
int  crgpu_dict_create(crgpu_ctx* ctx, const char* dictionary_text, crgpu_dict** out);
void crgpu_dict_destroy(crgpu_dict* dict);
int  crgpu_dict_words(const crgpu_dict* dict);          /* dictionary_load's return value */
int crgpu_dict_encode_blocks_dev(crgpu_ctx* ctx, crgpu_dict* dict,
                                 const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                                 uint32_t nblocks, uint32_t max_block,
                                 uint8_t* out, const uint64_t* out_off, uint32_t* out_size, int sync);
int crgpu_dict_decode_blocks_dev(crgpu_ctx* ctx, crgpu_dict* dict,
                                 const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                                 uint32_t nblocks, uint32_t max_block,
                                 uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                                 uint32_t* out_size, int sync);
/* Bytes dictionary_decode will produce for each dictionary-stage block (the sizes recorded at the end of its pieces,
 * src/cr-diccode.c:359-360, or n - 1 for the raw form): what a decoder needs to lay its output out before it runs.
 * out_size[b] = 0xFFFFFFFF for a malformed block. Device pointers. */
int crgpu_dict_decoded_sizes_dev(crgpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                                 uint32_t nblocks, uint32_t* out_size, int sync);
int crgpu_dict_encode_blocks(crgpu_ctx* ctx, crgpu_dict* dict,
                             const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                             uint32_t nblocks, uint8_t* out, const uint64_t* out_off, uint32_t* out_size);
int crgpu_dict_decode_blocks(crgpu_ctx* ctx, crgpu_dict* dict,
                             const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                             uint32_t nblocks, uint8_t* out, const uint64_t* out_off,
                             const uint32_t* out_cap, uint32_t* out_size);

/* ---- a dictionary per sequence of blocks (many files at once) ---------------------------------
 * crgpu_dict_set: ndict dictionaries made in one call, their tries built ON THE DEVICE (csrc/crgpu_dictset.h): the host only
 * parses the lines, the words of all dictionaries go up in one copy, and the node counts come back once to size the tries.
 * Device memory per dictionary: nodes x (512 + 4) bytes of trie (~40 MB for a dictionary of 25 000 words) plus
 * (words + 1) x 25 bytes of words; without a trie the words alone. The set also owns the encode scratch of its calls.
 *   texts[i]: dictionary text as dicpick() writes it (one word per line, NUL-terminated). with_trie = 0: words only, as
 *   dictionary_load(text, 0): such a set decodes and refuses to encode.
 * The stage calls give sequence s of blocks dictionary s of the set, all sequences in one launch per kernel. Pointer
 * conventions of crgpu_dict_encode_blocks_dev / _decode_blocks_dev; seq_first: HOST memory, nseq + 1 entries, ascending;
 * sequence s owns blocks seq_first[s] .. seq_first[s+1]-1 of the flat block arrays (it may own none). Coded bytes are those of
 * crgpu_dict_*_blocks with the sequence's dictionary; decode failures as there (0xFFFFFFFF per bad block, CRGPU_E_CORRUPT
 * when sync). The variants without _dev take HOST pointers and stage as crgpu_dict_encode_blocks / _decode_blocks do.
 * CRGPU_E_ARG: ndict == 0, a text of more than 25 000 lines, i >= ndict (_words / _nodes return it), nseq above the set's
 * size, a descending seq_first, a set of another context, an encode call on a set made without tries,
 * max_block > CRGPU_MAX_BLOCK + 1. */
typedef struct crgpu_dict_set crgpu_dict_set;
int  crgpu_dict_set_create(crgpu_ctx* ctx, const char* const* texts, uint32_t ndict, int with_trie, crgpu_dict_set** out);
void crgpu_dict_set_destroy(crgpu_dict_set* set);
int  crgpu_dict_set_words(const crgpu_dict_set* set, uint32_t i);   /* dictionary_load's return value for texts[i]  */
int  crgpu_dict_set_nodes(const crgpu_dict_set* set, uint32_t i);   /* trie nodes incl. the root; 0 without a trie */
int crgpu_dict_encode_sequences_dev(crgpu_ctx* ctx, crgpu_dict_set* set,
                                    const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                                    const uint32_t* seq_first, uint32_t nseq, uint32_t max_block,
                                    uint8_t* out, const uint64_t* out_off, uint32_t* out_size, int sync);
int crgpu_dict_decode_sequences_dev(crgpu_ctx* ctx, crgpu_dict_set* set,
                                    const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                                    const uint32_t* seq_first, uint32_t nseq, uint32_t max_block,
                                    uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                                    uint32_t* out_size, int sync);
int crgpu_dict_encode_sequences(crgpu_ctx* ctx, crgpu_dict_set* set,
                                const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                                const uint32_t* seq_first, uint32_t nseq,
                                uint8_t* out, const uint64_t* out_off, uint32_t* out_size);
int crgpu_dict_decode_sequences(crgpu_ctx* ctx, crgpu_dict_set* set,
                                const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size,
                                const uint32_t* seq_first, uint32_t nseq,
                                uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_size);

/* ---- several GPUs of one node (csrc/crgpu_multi.hip) -------------------------------------------------
 * The block loop of src/main.c:174-206 (encode) / :263-292 (decode) for INDEPENDENT datablocks, sharded over G devices:
 * one host thread, context and stream per device; rank r codes the contiguous block range [r*ceil(n/G), (r+1)*ceil(n/G));
 * each rank lays its run of the container out on its device (k_pack) and copies it to its offset of the output. The one
 * exchange is the per-block size table: ncclAllGather (RCCL) over a communicator of the devices, or — when the device
 * list names a GPU twice, holds a single device, or CRGPU_MULTI_HOST_GATHER is given — through host memory (the ranks
 * are threads). A rank whose range is empty (nblocks < G, or the tail of ceil(n/G) ranges) contributes zeros. */
typedef struct crgpu_multi crgpu_multi;
#define CRGPU_MULTI_DICT        1   /* run the dictionary stage (needs crgpu_multi_set_dictionary)                   */
#define CRGPU_MULTI_PREC        2   /* encode: dictionary stage only, no codec (the reference's -p; needs _DICT)     */
#define CRGPU_MULTI_HEADERS     4   /* encode: write the container's 6-byte block headers, skip empty blocks         */
#define CRGPU_MULTI_HOST_GATHER 8   /* crgpu_multi_create: exchange the size table through host memory, not RCCL     */
#define CRGPU_MULTI_RCCL       16   /* crgpu_multi_create with ONE device: still form the (one-rank) RCCL communicator;
                                       without it a single device exchanges nothing and librccl is not loaded        */
#define CRGPU_MULTI_PINNED_OUT 32   /* crgpu_multi_create: *out of the encode / decode calls lies in the context's page-locked pool
                                       (grown as needed, kept for the context's life): the ranks copy their runs out as DMA at the
                                       link's rate instead of staging them into fresh pageable memory. The result then belongs
                                       to the context: valid until the next job on it, crgpu_multi_free is a no-op for it.
                                       What the write loop src/main.c:198-205 / :281-292 needs: the bytes once, to fwrite them */
int  crgpu_multi_create(crgpu_multi** out, const int* devices, int ndev, int flags);
int  crgpu_multi_reserve_output(crgpu_multi* m, uint64_t bytes);   /* CRGPU_MULTI_PINNED_OUT: page-lock the pool ahead of the first job */
void crgpu_multi_destroy(crgpu_multi* m);
const char* crgpu_multi_last_error(const crgpu_multi* m);
int  crgpu_multi_devices(const crgpu_multi* m);
int  crgpu_multi_uses_rccl(const crgpu_multi* m);       /* 1: the size table travels by ncclAllGather                 */
/* Wall-clock marks of `rank` in the most recent job, in seconds since the job was handed to the ranks: [1] input on the
 * device (H2D done), [2] stages done (dictionary stage, codec, k_pack), [3] sizes exchanged, [4] output allocated,
 * [5] this rank's run copied out (D2H done). Returns CRGPU_MULTI_TIMES. What `comp*-gpu -t` prints. */
#define CRGPU_MULTI_TIMES 6
int  crgpu_multi_timing(const crgpu_multi* m, int rank, double* seconds, int room);
/* The deadline of a job (crgpu_multi_encode_blocks / _decode_blocks), in seconds; default 120, $CRGPU_MULTI_DEADLINE_S read
 * at crgpu_multi_create, 0 = wait for ever. A rank that never reaches the size exchange (a kernel that does not end, a device
 * that dropped out, a peer missing from ncclAllGather) would leave the others waiting in the collective for ever; instead the
 * call returns CRGPU_E_NODEVICE when the deadline passes, crgpu_multi_last_error names the ranks that did not arrive and
 * where they are stuck, and the context is abandoned: every later call on it fails, crgpu_multi_destroy leaves its threads
 * alone — they may still be reading the job's input, which therefore has to stay valid (a process that gets this error is
 * expected to report it and end, as the reference's only error path does: `perror + return -1`, src/main.c:207-214). */
int  crgpu_multi_set_deadline(crgpu_multi* m, double seconds);
int  crgpu_multi_set_dictionary(crgpu_multi* m, const char* dictionary_text);   /* dictionary_load on every device    */
int  crgpu_multi_configure(crgpu_multi* m, uint32_t rox_chain_limit, int flexible);   /* -m (0 = keep) / -f          */
/* HOST pointers. Block b = in[in_off[b] .. +in_size[b]). *out is allocated by the library (release it with
 * crgpu_multi_free) and holds the blocks' results in block order, *out_total bytes; out_off[b] / out_size[b]
 * (optional, nblocks entries) = position and size of block b's result in it.
 *   encode: result = lzencode(dictionary_encode(block)) (flags pick the stages), behind its block header with
 *           CRGPU_MULTI_HEADERS (filt[b] = the header's m_filt, NULL = 0);
 *   decode: in = the coded blocks (payloads, without container headers), prec[b] != 0 marks a block that only went
 *           through the dictionary stage; result = dictionary_decode(lzdecode(block)). */
int  crgpu_multi_encode_blocks(crgpu_multi* m, int codec, int flags,
                               const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size, uint32_t nblocks,
                               const uint8_t* filt, uint8_t** out, uint64_t* out_total, uint64_t* out_off, uint32_t* out_size);
int  crgpu_multi_decode_blocks(crgpu_multi* m, int codec, int flags,
                               const uint8_t* in, const uint64_t* in_off, const uint32_t* in_size, uint32_t nblocks,
                               const uint8_t* prec, uint8_t** out, uint64_t* out_total, uint64_t* out_off, uint32_t* out_size);
void crgpu_multi_free(void* p);
/* Host twins of the planning, used by the driver itself: rank's block range, and the exclusive sum of the slots
 * (6-byte header + payload for non-empty blocks when with_headers; entries of 0xFFFFFFFF count as 0). Returns the total. */
void crgpu_shard_range(uint32_t nblocks, int nranks, int rank, uint32_t* first, uint32_t* count);
uint64_t crgpu_container_offsets(const uint32_t* sizes, uint32_t nblocks, int with_headers, uint64_t* out_off);

/* Diagnostics: when dev_stats (device memory, 16 x uint64 per block of the next batches) is set,
 * every block records 100 MHz phase stamps [start, lzp-reset, lzp-scan, lzp-done, model-ready,
 * coded] plus its order-2 node and token counts. NULL switches it off again. */
int crgpu_debug_stats(crgpu_ctx* ctx, uint64_t* dev_stats);

/* Wave-primitive self test used by tests/: in = 66 uint32 (64 lane values, mask limit, table
 * index), out = 448 uint32 (scan, sum, byte-sum, mask, previous-equal-lane, table byte,
 * agreement flags of the three previous-equal-lane implementations). */
int crgpu_selftest(crgpu_ctx* ctx, const uint32_t* in, uint32_t* out);

/* ---- drop-in data_block_t + codec entry points (reference signatures, void, global state) ---- */
typedef struct data_block_t {
    uint8_t* m_data;
    uint32_t m_size;
    uint32_t m_capacity;
} data_block_t;

void data_block_reserve(data_block_t* block, uint32_t size);
void data_block_resize(data_block_t* block, uint32_t size);
void data_block_add(data_block_t* block, uint8_t byte);
void data_block_destroy(data_block_t* block);

/* Which reference binary the three shims below mirror. Without a call to crgpu_shim_config the codec follows the
 * front-end the library is linked into: every front-end defines `const char* cr_magic_header` (src/main.c:47;
 * src/roxmain/main.c:35 "...-comprox", src/rolzmain/main.c:35 "...-comprolz", src/ropmain/main.c:35 "...-comprop"),
 * the library holds a weak reference to it and picks the codec from its tail at the first shim call (comprop when
 * no such symbol exists). crgpu_shim_config (new, optional) overrides that and picks the device (default 0). */
int  crgpu_shim_config(int codec, int device);
int  crgpu_shim_codec(void);                          /* the codec the shims use (CRGPU_CODEC_*) */
/* Optional: bring the shims' device side up now (HIP runtime, context) rather than inside the first lzencode / lzdecode —
 * a tool calls it from the thread that is idle while dicpick() runs. Returns CRGPU_OK or the failure's code. */
int  crgpu_shim_prepare(void);
/* Optional hint: more blocks will follow WITHOUT reset_models() (the stock loop on a file of several blocks,
 * src/main.c:174-206). A block that starts from fresh models then runs on the model-carrying coder at once, so that its
 * successor continues from its models instead of rebuilding them from a second pass over its input. Same bytes either way. */
void crgpu_shim_expect_dependent_blocks(int on);
/* Opt-in (also: CRGPU_SHIM_PIPELINE_CARRY=1 in the environment, read at the first shim call): comprop's lzencode runs every
 * block through crgpu_encode_blocks_carried with one process-wide crgpu_models, whether the block starts fresh or continues the
 * last one; reset_models() resets the store; no input is remembered or replayed. An lzdecode that would have to continue
 * models the store holds reports CRGPU_E_ARG through the error hook (decoding dependent blocks stays on the one-wave coder:
 * leave the switch off in a process that does both). Off, the default: nothing changes. */
void crgpu_shim_pipeline_carry(int on);
float crgpu_shim_last_kernel_ms(void);                /* kernel time of the most recent lzencode / lzdecode call, -1 if none */
/* Page-locked host memory for buffers handed to the host-pointer entry points (DMA at the link's rate instead of the
 * runtime's staging of pageable memory); release with crgpu_host_free. NULL when it cannot be had. */
void* crgpu_host_alloc(size_t bytes);
void  crgpu_host_free(void* p);
/* The switches the reference's front-ends assign directly (src/roxmain/main.c:88,99, src/rolzmain/main.c:87;
 * extern in src/roxmain/cr-matcher.h:52,56 and src/rolzmain/cr-matcher.h:43): data symbols of the library,
 * read by the shims at every call. */
extern int      flexible_parsing;                     /* -f, comprox / comprolz; default 0 */
extern uint32_t match_limit;                          /* -m, comprox; default 40 */
int  crgpu_shim_rox_chain_limit(uint32_t limit);      /* = match_limit = limit */
int  crgpu_shim_flexible_parsing(int on);             /* = flexible_parsing = on */
/* Failures of the void entry points below (no gfx950 device, HIP error, malformed block): recorded, handed to the
 * handler, and the entry point returns with an empty output block. Without a handler: message to stderr and
 * exit(EXIT_FAILURE) — there is no CPU fallback, and carrying on would write a broken file. */
typedef void (*crgpu_error_fn)(int code, const char* message, void* user);
void crgpu_shim_set_error_handler(crgpu_error_fn fn, void* user);
int  crgpu_shim_status(void);                         /* CRGPU_OK or the code of the last failing shim call */
const char* crgpu_shim_last_error(void);

void reset_models(void);
void lzencode(data_block_t* ib, data_block_t* ob, int print_information);
void lzdecode(data_block_t* ib, data_block_t* ob, int print_information);

/* Static-dictionary entry points with the reference's signatures (src/cr-diccode.h:44-48,
 * src/cr-dicpick.h:40-42). dictionary_* run on the GPU through one process-wide crgpu_dict;
 * dicpick / dic_lcp_* are the once-per-file host passes and stay on the CPU. */
int  dictionary_load(const char* dicstr, int init_trie);
void dictionary_encode(data_block_t* i_block, data_block_t* o_block);
void dictionary_decode(data_block_t* i_block, data_block_t* o_block, FILE* fpout_sync);
void dicpick(FILE* fp, data_block_t* dic_block);
void dic_lcp_encode(data_block_t* dic_block);
void dic_lcp_decode(data_block_t* dic_block);

/* dicpick() for a stream that lies in device memory: the word census of src/cr-dicpick.c:164-226 as HIP kernels
 * (csrc/crgpu_dicpick.h) on the context's stream, the tail (:227-257) on the host over the kept words. dic_block receives
 * exactly the bytes dicpick() appends for a file holding the same n bytes; n <= 2^32 - 1 (CRGPU_E_ARG above). The call
 * returns when dic_block is complete. info (may be NULL): tokens = words counted, distinct = different words among them,
 * purges = how often the reference's map would have forgotten its little-used words (:115-144; replayed on the device,
 * one epoch per purge), fell_back = 1 when more than CRGPU_OPT_DICPICK_EPOCHS purges made the call copy the stream to
 * the host and run dicpick() there (same bytes; tokens / distinct then describe the device's scan, purges the cap),
 * kernel_ms = from the first kernel to the last on the stream. Device memory: 30 bytes per token + 8 per 8 192 bytes
 * of the stream, held by the context. crgpu_dicpick: the same from HOST memory (one copy to the device first). */
typedef struct { uint32_t tokens, distinct, purges, fell_back; float kernel_ms; } crgpu_dicpick_info;
int crgpu_dicpick_dev(crgpu_ctx* ctx, const uint8_t* dev_src, uint64_t n, data_block_t* dic_block, crgpu_dicpick_info* info);
int crgpu_dicpick(crgpu_ctx* ctx, const uint8_t* host_src, uint64_t n, data_block_t* dic_block, crgpu_dicpick_info* info);

/* `-F` pre-filters with the reference's signature (src/cr-filter.h:35-38; called per datablock by the
 * block loop, src/main.c:183-185 before dictionary_encode and :284-286 after dictionary_decode).
 * E8/E9 call-target conversion inside PE / ELF i386 images and colour + row + column deltas of 24/32-bit
 * BMP pixel arrays; host C (stateful across the blocks of a file, one cheap pass). Returns 1 when a
 * filter touched the block (the block header's m_filt). The state that carries an image from one block to
 * the next lives for the process, as in the reference; crgpu_filter_reset() (new) clears it. */
#define FILTER_ENC 0
#define FILTER_DEC 1
int  filter_inplace(unsigned char* buf, uint32_t len, int en_de);
void crgpu_filter_reset(void);
/* filter_inplace reproduces the reference's bytes by default, including elf_i386_transform's never-reset byte counter
 * (src/filter_x86_elf.c:131-134), which converts every ELF image after the first of a run in a way its own FILTER_DEC
 * cannot undo. CRGPU_FILTER_RESTART_ELF (new, NOT the reference's format) restarts the counter per image so that the
 * transform round-trips; comp*-gpu -FF selects it and marks such blocks with m_filt = 2 so that the decoder follows. */
#define CRGPU_FILTER_REFERENCE   0
#define CRGPU_FILTER_RESTART_ELF 1
int  crgpu_filter_set_mode(int mode);
int  crgpu_filter_mode(void);
/* How many ELF images filter_inplace has converted with the reference's stale counter (CRGPU_FILTER_REFERENCE, a second or
 * later ELF image of the run) since the last crgpu_filter_reset(): a stream for which this is not 0 does NOT come back
 * from FILTER_DEC — neither here nor in the reference. comp*-gpu -F prints a warning when it happens (also under -q). */
int  crgpu_filter_lossy(void);

/* filter_inplace for blocks that lie in device memory (csrc/crgpu_filter.h): after the call dev_data holds exactly the
 * bytes that filter_inplace(data + off[b], len[b], en_de) leaves when called for b = 0..nb-1 in order, touched[b] (host
 * memory, nb entries) is that call's return value, and the process-wide filter state (the open image, the mode, the
 * lossy count) is what those calls leave: a stream may be fed in slices, host and device calls may be mixed,
 * crgpu_filter_reset() clears it for both. off is ascending, the blocks do not overlap, len[b] <= CRGPU_MAX_BLOCK
 * (CRGPU_E_ARG otherwise); nothing outside the blocks is read or written. The device finds and analyses the image
 * headers, the host walks the filters' state machines over what it found (a few decisions per image), the device
 * transforms — from a snapshot of the blocks (packed back to back: gaps between the blocks cost nothing), so the
 * context holds one byte of device memory per byte of the blocks plus 32 bytes per header found. The call returns when the stream is done. info (may be NULL): images = headers
 * that passed a filter's analysis, pieces = ranges transformed, fell_back = 1 when an ELF image's pass rewrote bytes
 * behind its claimed length that hold a header signature (before or after): the call then restored the stream and ran
 * filter_inplace on the host (same bytes); rescans is reserved (0); kernel_ms = the kernels' time (HIP events around each group
 * of kernels, summed; readbacks, the plan and the copies are not in it).
 * crgpu_filter_blocks: the same for HOST memory, one copy in and one out per run of adjacent blocks (staged back to back). */
typedef struct { uint32_t images, pieces, rescans, fell_back; float kernel_ms; } crgpu_filter_info;
int crgpu_filter_blocks_dev(crgpu_ctx* ctx, uint8_t* dev_data, const uint64_t* off, const uint32_t* len, uint32_t nb,
                            int en_de, uint8_t* touched, crgpu_filter_info* info);
int crgpu_filter_blocks(crgpu_ctx* ctx, uint8_t* host_data, const uint64_t* off, const uint32_t* len, uint32_t nb,
                        int en_de, uint8_t* touched, crgpu_filter_info* info);

#ifdef __cplusplus
}
#endif
#endif
