/*
 * mfm_runsync.h - what the kernels of the burst sync stage (mfm_runsync_*, include/multifm_hip.h) and its host twin
 * (mfm_hosttwin_runsync_call) must state once: the bit of a decision, the register a window of bits stands for, the match of a
 * register against the table of sync words, what a run starts from and leaves behind, and what a stored state must satisfy.  The
 * checks a run has to pass before a decision is read are mfm_run_stage.h's: struct mfm_runmm_run has the field layout of struct
 * mfm_runrs_run (dec_offset for out_offset, first_dec for first_out, nr_dec for nr_out) and the state below that of a state with
 * `outs` where it has `decs`, so mfm_run_check_run reads both as they are.
 *
 * The register.  The reference's consumer (pager/test/test_mueller_muller.c:130-136) shifts every bit in at the bottom of a 32-bit
 * register: after decision n, bit k of the register is the bit of decision n - k, and 0 where the stretch has no such decision.
 * The stage packs bits the other way round, as the burst resampler's bits form does: decision j of a run is bit j % 32 of the
 * run's word j / 32.  The 32 bits that end in decision j are therefore a 64-bit funnel of two neighbouring words shifted right by
 * (j + 1) % 32 (mfm_runsync_window), and the register is those 32 bits reversed.  In front of a run's first word stands the seed
 * word: the carried register reversed where the run continues a stretch, 0 where it begins one.
 */
#ifndef MFM_RUNSYNC_H
#define MFM_RUNSYNC_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/multifm_hip.h"
#include "mfm_run_stage.h"

#define MFM_RUNSYNC_SEGMENT 1024u /* decisions of a run one wave packs and matches (rsy_match_kernel, mfm_runsync.hip) */

static_assert(MFM_RUNSYNC_IN_RUNMM == MFM_RUN_IN_RUNRS && MFM_RUNSYNC_IN_OUT_OF_STEP == MFM_RUN_IN_OUT_OF_STEP &&
                  MFM_RUNSYNC_IN_BAD_RUNS == MFM_RUN_IN_BAD_RUNS && MFM_RUNSYNC_OVER_RUNS == MFM_RUN_OVER_RUNS,
              "the burst stages share the values of their flags");
static_assert(sizeof(mfm_runmm_run) == sizeof(mfm_runrs_run) && offsetof(mfm_runmm_run, dec_offset) == offsetof(mfm_runrs_run, out_offset) &&
                  offsetof(mfm_runmm_run, first_dec) == offsetof(mfm_runrs_run, first_out) &&
                  offsetof(mfm_runmm_run, channel) == offsetof(mfm_runrs_run, channel) &&
                  offsetof(mfm_runmm_run, nr_dec) == offsetof(mfm_runrs_run, nr_out) && offsetof(mfm_runmm_run, flags) == offsetof(mfm_runrs_run, flags),
              "struct mfm_runmm_run has the field layout of struct mfm_runrs_run");

/* struct mfm_runsync_state as mfm_run_check_run reads a state: the decisions are the stretch's outputs so far */
struct __attribute__((may_alias)) mfm_runsync_state_outs {
    uint64_t stretch_window, outs;
    uint32_t shr, has_stretch;
};
static_assert(sizeof(mfm_runsync_state) == 24 && sizeof(mfm_runsync_state_outs) == 24 &&
                  offsetof(mfm_runsync_state, decs) == offsetof(mfm_runsync_state_outs, outs) &&
                  offsetof(mfm_runsync_state, has_stretch) == offsetof(mfm_runsync_state_outs, has_stretch),
              "struct mfm_runsync_state is 24 bytes");
typedef mfm_runrs_run __attribute__((may_alias)) mfm_runsync_in_run; /* a struct mfm_runmm_run, read through the shared checks */

/* the table a register is held against, as create takes it */
struct mfm_runsync_params {
    uint32_t words[8];
    uint32_t nr_words, max_distance, bit_rule, either;
};

/* mfm_run_totals_check on the Mueller-Muller stage's totals: more decisions than the capacity is an overflow of this stage, not a
 * list that cannot be (before a run is looked at, MFM_RUN_IN_BAD_RUNS can only mean that) */
__host__ __device__ inline void mfm_runsync_totals_check(const uint64_t *mtotals, uint64_t cap_decs, uint64_t cap_runs, uint64_t *n, uint64_t *E,
                                                         uint64_t *over, uint64_t *err)
{
    mfm_run_totals_check(mtotals, cap_decs, cap_runs, n, E, over, err);
    if (*err == MFM_RUN_IN_BAD_RUNS) {
        *err = 0;
        *over = MFM_RUNSYNC_OVER_DECISIONS;
    }
}

/* create's conditions on the table; NULL when they hold, else what is wrong */
inline const char *mfm_runsync_params_check(const mfm_runsync_config &cfg, mfm_runsync_params *out)
{
    if (cfg.nr_words < 1u || cfg.nr_words > 8u) {
        return "nr_words must be 1 .. 8";
    }
    if (cfg.max_distance > 15u) {
        return "max_distance must be at most 15: beyond it a register can match a word and its complement at once";
    }
    if (cfg.bit_rule != MFM_RUNSYNC_BIT_NOT_POS && cfg.bit_rule != MFM_RUNSYNC_BIT_POS) {
        return "bit_rule must be MFM_RUNSYNC_BIT_NOT_POS or MFM_RUNSYNC_BIT_POS";
    }
    if (cfg.flags & ~MFM_RUNSYNC_F_EITHER) {
        return "flags must be 0 or MFM_RUNSYNC_F_EITHER";
    }
    if (out) {
        for (uint32_t k = 0; k < 8u; k++) {
            out->words[k] = k < cfg.nr_words ? cfg.words[k] : 0u;
        }
        out->nr_words = cfg.nr_words;
        out->max_distance = cfg.max_distance;
        out->bit_rule = cfg.bit_rule;
        out->either = (cfg.flags & MFM_RUNSYNC_F_EITHER) ? 1u : 0u;
    }
    return nullptr;
}

/* the bit of a decision: !(d > 0) is the reference's (:132), which differs from a sign bit at d == 0 alone */
__host__ __device__ inline uint32_t mfm_runsync_bit(int32_t d, uint32_t bit_rule)
{
    return bit_rule == MFM_RUNSYNC_BIT_POS ? (d > 0 ? 1u : 0u) : (d > 0 ? 0u : 1u);
}

__host__ __device__ inline uint32_t mfm_runsync_popcount(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(v);
#else
    return (uint32_t)__builtin_popcount(v);
#endif
}

__host__ __device__ inline uint32_t mfm_runsync_reverse(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(v);
#else
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    return (v >> 16) | (v << 16);
#endif
}

/* the 32 packed bits that end `shift` bits into hi (shift 0 .. 32): the funnel of two neighbouring words */
__host__ __device__ inline uint32_t mfm_runsync_window(uint32_t lo, uint32_t hi, uint32_t shift)
{
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> shift);
}

/*
 * The register after decision j of a run from the run's packed words: bits[] are the run's nw words, seed the word in front of
 * them.  For j < 31 the window reaches into the seed.
 */
__host__ __device__ inline uint32_t mfm_runsync_register_at(const uint32_t *bits, uint32_t nw, uint32_t seed, uint32_t j)
{
    const uint32_t p = j + 1u; /* the window is bits [p - 32, p) of the run, the seed being bits [-32, 0) */
    const uint32_t w = p >> 5;
    const uint32_t lo = w == 0u ? seed : bits[w - 1u];
    const uint32_t hi = w < nw ? bits[w] : 0u;
    return mfm_runsync_reverse(mfm_runsync_window(lo, hi, p & 31u));
}

/* a register against the table (:134 with several words and the complement): the lowest word index that matches, the word
 * before its complement; false when none does */
__host__ __device__ inline bool mfm_runsync_match(uint32_t shr, const mfm_runsync_params &P, uint32_t *word_index, uint32_t *distance,
                                                  uint32_t *inverted)
{
#pragma unroll /* over the table's eight places: the words stay in registers, no place of the table is addressed */
    for (uint32_t k = 0; k < 8u; k++) {
        if (k >= P.nr_words) {
            break;
        }
        const uint32_t d = mfm_runsync_popcount(P.words[k] ^ shr);
        if (d <= P.max_distance) {
            *word_index = k;
            *distance = d;
            *inverted = 0;
            return true;
        }
        if (P.either && 32u - d <= P.max_distance) { /* popcount(~word ^ shr) */
            *word_index = k;
            *distance = 32u - d;
            *inverted = 1;
            return true;
        }
    }
    return false;
}

/* what a run starts from: its channel's state where it continues a stretch, an empty register where it begins one */
__host__ __device__ inline mfm_runsync_state mfm_runsync_start(const mfm_runsync_state &old, uint64_t first_window, uint32_t flags)
{
    if (!(flags & MFM_RUNRS_BEGINS)) {
        return old;
    }
    mfm_runsync_state st;
    st.stretch_window = first_window;
    st.decs = 0;
    st.shr = 0;
    st.has_stretch = 1;
    return st;
}

/* What a state handed in from outside (mfm_runsync_store_state) must satisfy before a kernel reads it; NULL when it does, else
 * a message that names the field.  A register holds no bit of a decision the stretch has not had. */
inline const char *mfm_runsync_state_check(const mfm_runsync_state &st)
{
    if (st.has_stretch > 1u) {
        return "has_stretch must be 0 or 1";
    }
    if (!st.has_stretch) {
        return st.stretch_window || st.decs || st.shr ? "has_stretch is 0 but another field is not 0" : nullptr;
    }
    if (st.decs >= MFM_RUN_POS_LIMIT || st.stretch_window >= MFM_RUN_POS_LIMIT) {
        return "decs and stretch_window must be below 2^62";
    }
    if (st.decs < 32u && (st.shr >> st.decs) != 0u) {
        return "shr must hold no bit at or above bit decs while decs is below 32";
    }
    return nullptr;
}

#endif /* MFM_RUNSYNC_H */
