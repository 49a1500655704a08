/*
 * mfm_gate_internal.h - what mfm_gate.hip (the gate, its five kernels) and mfm_gate_preroll.hip (the pre-roll mode: its
 * kernels, the setter, the flush and the host twin) share: the stage object and three hidden entry points.
 */
#ifndef MFM_GATE_INTERNAL_H
#define MFM_GATE_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/multifm_hip.h"

constexpr uint32_t MFM_GT_PIECE = 8192; /* elements one group of the copy kernels copies at most: 256 lanes, 4 chunks of 8 each */
constexpr uint32_t MFM_GT_T_RUNS = 0, MFM_GT_T_ELEMS = 1, MFM_GT_T_OVERFLOW = 2, MFM_GT_T_OUT_OF_STEP = 3; /* d_totals[] */

struct mfm_gate {
    mfm_gate_config cfg{};
    uint32_t W = 0, E = 1, We = 0;
    uint32_t max_win = 0;      /* windows per channel and call at most */
    uint64_t cap_windows = 0;  /* payload capacity, windows */
    uint64_t cap_runs = 0;
    uint32_t carry_stride = 0;
    uint32_t log2g = 0, npieces = 1;
    uint64_t pos = 0;          /* samples per channel consumed so far */
    int16_t *d_carry = nullptr;
    uint32_t *d_cnt_open = nullptr, *d_cnt_runs = nullptr, *d_bad = nullptr, *d_base_runs = nullptr, *d_base_open = nullptr, *d_slot = nullptr;
    uint64_t *d_totals = nullptr;
    mfm_gate_run *d_runs = nullptr;
    int16_t *d_payload = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_call = false;
    /* pre-roll (mfm_gate_preroll.hip); all unused while P == 0 */
    uint32_t P = 0;
    uint32_t slot_stride = 0;  /* of d_slot: max(max_win, P) once the setter ran */
    uint32_t hist_stride = 0;  /* elements per channel of either history buffer */
    int16_t *d_hist[2] = { nullptr, nullptr }; /* used in turn: a call reads [cur] and writes [cur ^ 1] */
    uint64_t *d_bits[2] = { nullptr, nullptr }; /* the open bits of the P records in front of the next call, likewise */
    uint32_t cur = 0;
    bool flushed = false;
};

extern "C" {
__attribute__((visibility("hidden"))) void mfm_internal_set_error(const char *msg);
/* mfm_gate.hip: set the thread's message, return code */
__attribute__((visibility("hidden"))) int mfm_gate_internal_fail(int code, const char *msg);
/* mfm_gate.hip: queue gt_scan_kernel over d_cnt_open / d_cnt_runs / d_bad */
__attribute__((visibility("hidden"))) int mfm_gate_internal_scan(struct mfm_gate *g, hipStream_t s);
/* mfm_gate_preroll.hip: one process call (flush == 0) or the flush of a gate whose P > 0; arguments checked by the caller */
__attribute__((visibility("hidden"))) int mfm_gate_internal_preroll_call(struct mfm_gate *g, const int16_t *d_rows, size_t in_stride, size_t nr_in,
                                                                       const struct mfm_level_record *d_records, size_t record_stride,
                                                                       uint32_t nwin, int flush, hipStream_t s);
}

#endif /* MFM_GATE_INTERNAL_H */
