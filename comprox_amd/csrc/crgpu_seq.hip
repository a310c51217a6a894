/*
 * comprox_amd/csrc/crgpu_seq.hip — the kernels of crgpu_seq.h (many sequences of dependent comprop blocks in lockstep) and of
 * crgpu_seq_lz.h (the same for comprox and comprolz) as a translation unit of their own, and their launchers; the host side
 * of the feature is in crgpu.hip.
 */
#include <hip/hip_runtime.h>

#define CRGPU_CARRY_FUNCS
#define CRGPU_SEQ_TU
#include "crgpu_seq_lz.h"

void crs_launch_fill(hipStream_t s, uint32_t grid, uint8_t* store, const uint32_t* which, uint32_t n) {
    hipLaunchKernelGGL(k_seq_fill, dim3(grid, n), dim3(256), 0, s, store, which);
}
void crs_launch_gather(hipStream_t s, const uint32_t* map, uint32_t n, const u64* in_off, const uint32_t* in_size, const u64* out_off,
                       u64* d_in_off, uint32_t* d_in_size, u64* d_out_off) {
    hipLaunchKernelGGL(k_seq_gather, dim3((n + 255u) / 256u), dim3(256), 0, s, map, n, in_off, in_size, out_off, d_in_off, d_in_size, d_out_off);
}
void crs_launch_scatter(hipStream_t s, const uint32_t* map, uint32_t n, const uint32_t* d_out_size, uint32_t* out_size) {
    hipLaunchKernelGGL(k_seq_scatter, dim3((n + 255u) / 256u), dim3(256), 0, s, map, n, d_out_size, out_size);
}
void crs_launch_events(hipStream_t s, const CrBatch& B, const CrArenaLayout& L, const CrSeq& Q) { hipLaunchKernelGGL(k_seq_events, dim3(B.nblocks), dim3(CRGPU_WAVE), 0, s, B, L, Q); }
void crs_launch_o3(hipStream_t s, uint32_t grid_x, const CrBatch& B, const CrSeq& Q) { hipLaunchKernelGGL(k_seq_o3, dim3(grid_x, B.nblocks), dim3(256), 0, s, B, Q); }
void crs_launch_o2(hipStream_t s, uint32_t grid_x, const CrBatch& B, const CrSeq& Q) { hipLaunchKernelGGL(k_seq_o2, dim3(grid_x, B.nblocks), dim3(CR_O2C_THREADS), 0, s, B, Q); }
void crs_launch_o1(hipStream_t s, const CrBatch& B, const CrSeq& Q) { hipLaunchKernelGGL(k_seq_o1, dim3(B.nblocks), dim3(CR_O1_THREADS), 0, s, B, Q); }
void crs_launch_undo(hipStream_t s, const CrBatch& B, const CrSeq& Q) { hipLaunchKernelGGL(k_seq_undo, dim3(B.nblocks), dim3(256), 0, s, B, Q); }

void crs_launch_side_fill(hipStream_t s, uint8_t* keep, const uint32_t* which, uint32_t n, int rolz) { hipLaunchKernelGGL(k_seq_side_fill, dim3(n), dim3(CRGPU_WAVE), 0, s, keep, which, rolz); }
void crs_launch_lz_events(hipStream_t s, int rolz, const CrBatch& B, const CrArenaLayout& L, const CrSeq& Q, uint8_t* keep) {
    if (rolz) hipLaunchKernelGGL(k_seq_rolz_events, dim3(B.nblocks), dim3(CRGPU_WAVE), 0, s, B, L, Q, keep);
    else hipLaunchKernelGGL(k_seq_rox_events, dim3(B.nblocks), dim3(256), 0, s, B, L, Q, keep);
}
void crs_launch_lz_abort(hipStream_t s, int rolz, const CrBatch& B1, const CrArenaLayout& L, const CrSeq& Q1, uint8_t* keep) {
    if (rolz) hipLaunchKernelGGL(k_seq_lz_abort<true>, dim3(1), dim3(CRGPU_WAVE), 0, s, B1, L, Q1, keep);
    else hipLaunchKernelGGL(k_seq_lz_abort<false>, dim3(1), dim3(CRGPU_WAVE), 0, s, B1, L, Q1, keep);
}
void crs_launch_lz_stored(hipStream_t s, int rolz, const CrBatch& B, uint32_t* flags) { hipLaunchKernelGGL(k_seq_lz_stored, dim3((B.nblocks + 255u) / 256u), dim3(256), 0, s, B, rolz, flags); }
