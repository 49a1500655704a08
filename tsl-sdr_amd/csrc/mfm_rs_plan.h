/*
 * mfm_rs_plan.h - which kernel the PCM resampler (mfm_resampler.hip) runs and with what geometry, decided on the host from the
 * configuration and the taps alone, and the host tables that kernel reads.  No device pointers, no HIP runtime calls:
 * mfm_resampler_create() calls rs_plan() and rs_build_tables(), then uploads; mfm_hosttwin_resampler_form() runs the same
 * planner without a device.  The selection rules are stated at the head of mfm_resampler.hip, in the order applied here.
 */
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../../include/multifm_hip.h"

constexpr uint32_t RS_NT = 256, RS_OPT = 4, RS_OPB = RS_NT * RS_OPT; /* v_dot2 form: threads, outputs per thread / per block */
constexpr uint32_t RS_PAIRS_MAX = 32;                                /* register-resident phase: up to 64 taps */
constexpr uint32_t RSM_NT = 256; /* matrix form: threads per workgroup (4 waves) */
constexpr uint32_t RSM_NB = 256; /* blocks of 16 outputs per workgroup: each wave does four column groups of 16 blocks */
constexpr uint32_t RS_LDS_MAX = 150u * 1024u;     /* what a workgroup may ask for at all */
constexpr uint32_t RS_LDS_DEFAULT = 48u * 1024u;  /* above this a kernel's dynamic LDS limit is raised before its first launch */
constexpr uint32_t RSM_WINDOW_MAX = 256, RSM_R_MAX = 240;
constexpr int32_t RSM_TAP_MAX = 32639; /* W = 256 Wh + Wl with both in [-128, 127] */

struct RsPlan {
    uint32_t I = 0, D = 0, nr_coeffs = 0;
    uint32_t plen = 0;   /* taps per phase (filter/polyphase_fir.c:70-83, rounded up to a multiple of 4) */
    uint32_t in_cap = 0, out_cap = 0, tail_cap = 0;
    int32_t dc_p = 0;    /* filter/dc_blocker.h:56 */
    /* v_dot2 form */
    uint32_t lds_bytes = 0; /* coefficient pairs + the input window of RS_OPB outputs */
    bool reg_coef = false;  /* the thread's coefficient pairs in registers ... */
    uint32_t np = 0;        /* ... of the instance NP = 4, 8, ..., 32; 0: pairs read from LDS */
    /* matrix form */
    bool use_mfma = false;
    uint32_t fallback = MFM_RS_FB_NONE; /* MFM_RS_FB_*: why not */
    uint32_t ks = 0, R = 0, rp = 0, K = 0, m_plane = 0, m_lds = 0;
    char err[192] = "";
};

/* what mfm_resampler_create() refuses on its arguments, before it looks for a device */
inline bool rs_args_ok(const mfm_resampler_config &cfg, size_t nr_coeffs)
{
    return cfg.abi_version == MFM_ABI_VERSION && cfg.interpolate && cfg.decimate && cfg.nr_channels && cfg.max_in_samples && nr_coeffs;
}

/* MFM_OK, or MFM_E_INVAL (with plan.err set for the shapes no kernel here runs).  coeffs is not NULL. */
inline int rs_plan(const mfm_resampler_config &cfg, const int16_t *coeffs, size_t nr_coeffs, RsPlan &p)
{
    if (!rs_args_ok(cfg, nr_coeffs)) {
        return MFM_E_INVAL;
    }
    const uint32_t I = cfg.interpolate, D = cfg.decimate;
    p.I = I;
    p.D = D;
    p.nr_coeffs = (uint32_t)nr_coeffs;
    /* filter/polyphase_fir.c:70-83 */
    uint32_t plen = (uint32_t)((nr_coeffs + I - 1) / I);
    plen = (plen + 3u) & ~3u;
    p.plen = plen;
    /* the walk must not step past the samples it has (one output consumes at most ceil(D/I) samples) */
    if ((D + I - 1) / I > plen) {
        snprintf(p.err, sizeof(p.err), "resampling ratio %u/%u consumes up to %u samples per output, more than the %u taps of a phase",
                 I, D, (D + I - 1) / I, plen);
        return MFM_E_INVAL;
    }
    p.in_cap = cfg.max_in_samples + plen + 64;
    p.out_cap = (uint32_t)(((uint64_t)p.in_cap * I) / D + 8);
    p.out_cap = (p.out_cap + 7u) & ~7u; /* rows of the output start 16-byte aligned (the matrix-core form stores four outputs at
                                         * once, the DC blocker reads and writes eight) */
    if ((uint64_t)p.out_cap * D >= (1ull << 32)) {
        snprintf(p.err, sizeof(p.err), "%u outputs per call at decimation %u: the phase walk of a call does not fit 32 bits", p.out_cap, D);
        return MFM_E_INVAL;
    }
    p.tail_cap = plen + 8; /* never more than plen samples are left over (see rs_process) */
    if (cfg.dc_block) {
        p.dc_p = (int16_t)((1.0 - cfg.dc_pole) * 16384.0); /* filter/dc_blocker.h:56 */
    }
    /* LDS of a v_dot2 workgroup: coefficient pairs + the input window of RS_OPB outputs */
    p.lds_bytes = (uint32_t)((size_t)I * plen * 2 + (((uint64_t)RS_OPB * D) / I + plen + 32) * 2);
    p.lds_bytes = (p.lds_bytes + 15u) & ~15u;
    if (p.lds_bytes > RS_LDS_MAX) {
        snprintf(p.err, sizeof(p.err), "resampling ratio %u/%u with %u taps per phase needs %u bytes of LDS per workgroup", I, D, plen,
                 p.lds_bytes);
        return MFM_E_INVAL;
    }
    /* only extreme decimation ratios exceed the default limit: they use the LDS-coefficient variant */
    p.reg_coef = ((uint64_t)RS_NT * D) % I == 0 && plen / 2 <= RS_PAIRS_MAX && p.lds_bytes <= RS_LDS_DEFAULT;
    p.np = p.reg_coef ? ((plen / 2u + 3u) / 4u) * 4u : 0u; /* register variant: pairs rounded up to 4 */

    /* ---- matrix-core form: y[16 m + q] = sum_s G[q][s] x[R m + s], one G per carried phase ---- */
    p.fallback = MFM_RS_FB_NONE;
    if (cfg.flags & MFM_RS_FORCE_DOT2) {
        p.fallback = MFM_RS_FB_FORCED;
    } else if ((16u * (uint64_t)D) % I != 0u) {
        p.fallback = MFM_RS_FB_RATIO;
    } else if (16u * (uint64_t)D / I > RSM_R_MAX) {
        p.fallback = MFM_RS_FB_BLOCK;
    }
    if (MFM_RS_FB_NONE == p.fallback) {
        const uint32_t R = 16u * D / I, rp = (R + 15u) & ~15u;
        /* output q of a block starts its window floor((phi + q D) / I) samples into the block, phi < I */
        const uint32_t max_off = (I - 1u + 15u * D) / I;
        const uint32_t last = max_off + plen - 1u; /* last sample index (from the block's first) with a coefficient */
        uint32_t K = (last / R) * rp + last % R + 1u; /* its byte position in the padded rows, + 1 */
        K = (K + 63u) & ~63u;
        if (K > RSM_WINDOW_MAX) {
            p.fallback = MFM_RS_FB_WINDOW;
        } else {
            for (size_t i = 0; i < nr_coeffs; i++) {
                if (coeffs[i] < -RSM_TAP_MAX || coeffs[i] > RSM_TAP_MAX) {
                    p.fallback = MFM_RS_FB_TAP_RANGE;
                    break;
                }
            }
        }
        if (MFM_RS_FB_NONE == p.fallback) {
            p.use_mfma = true;
            p.ks = K / 64u;
            p.R = R;
            p.rp = rp;
            p.K = K;
            const uint32_t nrows = RSM_NB + (K + rp - 1u) / rp;
            p.m_plane = (nrows * rp + 63u) & ~63u;
            p.m_lds = 2u * p.m_plane;
        }
    }
    return MFM_OK;
}

inline void rs_plan_form(const RsPlan &p, mfm_resampler_form *f)
{
    *f = mfm_resampler_form{};
    f->form = p.use_mfma ? 1u : 0u;
    f->fallback = p.fallback;
    f->reg_pairs = p.use_mfma ? 0u : p.np;
    f->k_steps = p.ks;
    f->block_samples = p.R;
    f->row_bytes = p.rp;
    f->window_bytes = p.K;
    f->lds_bytes = p.use_mfma ? p.m_lds : p.lds_bytes;
    f->phase_len = p.plen;
    f->max_out = p.out_cap;
    f->dc_p = p.dc_p;
}

struct RsTables {
    std::vector<int16_t> phase; /* [I][plen] */
    std::vector<int8_t> frag;   /* matrix form: [I][2 planes: Wh, Wl][KS][64 lanes][16] A fragments of G, one G per carried phase */
    std::vector<int32_t> krow;  /* matrix form: [I][16], 128 * sum of row q of G (the x = ... + 128 term) */
};

/* every table the plan's kernel reads */
inline void rs_build_tables(const RsPlan &p, const int16_t *coeffs, RsTables &t)
{
    const uint32_t I = p.I, D = p.D, plen = p.plen;
    t.phase.assign((size_t)I * plen, 0);
    for (size_t i = 0; i < p.nr_coeffs; i++) {
        t.phase[(i % I) * plen + (i / I)] = coeffs[i];
    }
    t.frag.clear();
    t.krow.clear();
    if (!p.use_mfma) {
        return;
    }
    const uint32_t KS = p.ks, K = p.K, R = p.R, rp = p.rp;
    t.frag.assign((size_t)I * 2u * KS * 64u * 16u, 0);
    t.krow.assign((size_t)I * 16u, 0);
    for (uint32_t phi = 0; phi < I; phi++) {
        for (uint32_t q = 0; q < 16; q++) {
            const uint32_t tt = phi + q * D, off = tt / I, phq = tt % I;
            uint32_t sum = 0;
            for (uint32_t kk = 0; kk < K; kk++) {
                const uint32_t row = kk / rp, col = kk % rp;
                int32_t w = 0;
                if (col < R) {
                    const int64_t tap = (int64_t)(row * R + col) - (int64_t)off;
                    if (tap >= 0 && tap < (int64_t)plen) {
                        w = t.phase[(size_t)phq * plen + (size_t)tap];
                    }
                }
                sum += (uint32_t)w;
                const int32_t wl = (int8_t)(w & 0xff), wh = (w - wl) >> 8;
                /* v_mfma_i32_16x16x64_i8 A operand: lane (kg = lane >> 4, i = lane & 15) holds row i, elements 64 ks + 16 kg + j */
                const uint32_t ks = kk / 64u, kgq = (kk % 64u) / 16u, j = kk % 16u, ln = kgq * 16u + q;
                t.frag[((((size_t)phi * 2u + 0u) * KS + ks) * 64u + ln) * 16u + j] = (int8_t)wh;
                t.frag[((((size_t)phi * 2u + 1u) * KS + ks) * 64u + ln) * 16u + j] = (int8_t)wl;
            }
            t.krow[(size_t)phi * 16u + q] = (int32_t)(128u * sum);
        }
    }
}
