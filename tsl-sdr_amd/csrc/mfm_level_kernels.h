/*
 * mfm_level_kernels.h - what the level stage's two finish kernels share (lv_finish_kernel in mfm_level.hip, the fixed
 * thresholds; lv_adaptive_finish_kernel in mfm_level_adaptive.hip, the squelch on the channel's own noise floor): the call's
 * geometry, the per-slot partial sums the input kernels leave, the per-channel state, the sums of a round of 64 completed
 * windows and what a call leaves behind them.  Internal to the library; the arithmetic is mfm_level.h's.
 */
#ifndef MFM_LEVEL_KERNELS_H
#define MFM_LEVEL_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/multifm_hip.h"

namespace mfm_lv {

struct LvGeom {
    uint64_t P;      /* absolute element position of the call's first element */
    uint64_t g0;     /* absolute index of the first slot the call touches */
    uint32_t N;      /* elements per channel in this call */
    uint32_t We, B, nsub;
    uint32_t nslots; /* slots the call touches */
    uint32_t with_diff;
};

struct LvPart {
    uint64_t energy, diff;
    uint32_t peak, pad;
};

struct LvChan {
    uint64_t energy, diff; /* of the unfinished window */
    uint32_t peak;
    uint32_t prev;         /* last element of the stream so far (PCM form), as uint16 */
    uint32_t open, bad;
};

struct LvSquelch {
    uint64_t open_thr, close_thr;
    uint32_t use_diff, below, hang, pad;
};

struct LvFinish {
    LvGeom G;
    LvSquelch Q;
    const int16_t *x;
    size_t stride;
    LvChan *st;
    const LvPart *parts;
    uint32_t parts_stride;
    mfm_level_record *rec;
    uint32_t rec_stride;
    uint32_t *d_open;
    uint64_t k0;   /* window the call's first element lies in */
    uint32_t nwin; /* windows the call completes */
    uint32_t tail; /* 1: elements of an unfinished window are left behind them */
};

/* the adaptive squelch of one call: the setting, where the stream stands and the two buffers it adds */
struct LvAdaptive {
    uint32_t M, open_q8, close_q8, warmup;
    uint64_t done;      /* windows completed since create or the last seek, before this call */
    uint64_t *hist;     /* [channel][hist_stride]: the keys of the channel's last M - 1 windows, the newest last */
    uint64_t *floor;    /* [channel][floor_stride]: the floor of every window of the call */
    uint32_t hist_stride, floor_stride;
};

constexpr uint32_t LV_STRIP = 1024; /* windows of a call the adaptive kernel holds in LDS at a time */

__device__ __forceinline__ uint64_t lv_wave_sum(uint64_t v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        v += (uint64_t)__shfl_xor((unsigned long long)v, o);
    }
    return v;
}

__device__ __forceinline__ uint32_t lv_wave_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint32_t w = (uint32_t)__shfl_xor((int)v, o);
        v = w > v ? w : v;
    }
    return v;
}

/* the call's slots of window k: [lo, hi) as indices into the channel's parts */
__device__ __forceinline__ void lv_slots_of(const LvGeom &G, uint64_t k, uint32_t &lo, uint32_t &hi)
{
    const uint64_t f = k * G.nsub, e = f + G.nsub, g1 = G.g0 + G.nslots;
    lo = (uint32_t)((f > G.g0 ? f : G.g0) - G.g0);
    hi = (uint32_t)((e < g1 ? e : g1) - G.g0);
}

/* the sums of slots [lo, hi), every lane taking part; all lanes get the result */
__device__ __forceinline__ void lv_wave_slots(const LvPart *pc, uint32_t lane, uint32_t lo, uint32_t hi, uint64_t &e, uint64_t &d, uint32_t &p)
{
    uint64_t le = 0, ld = 0;
    uint32_t lp = 0;
    for (uint32_t j = lo + lane; j < hi; j += 64) {
        const LvPart t = pc[j];
        le += t.energy;
        ld += t.diff;
        lp = t.peak > lp ? t.peak : lp;
    }
    e = lv_wave_sum(le);
    d = lv_wave_sum(ld);
    p = lv_wave_max(lp);
}

/*
 * One round: the sums of the call's completed windows m0 .. m0 + cnt - 1 (cnt <= 64), lane j getting those of window m0 + j;
 * s is the channel's state as the call found it, whose sums belong to the call's first window.  The whole wave calls it.
 */
__device__ __forceinline__ void lv_round_sums(const LvFinish &L, const LvChan &s, const LvPart *pc, uint32_t lane, uint32_t m0, uint32_t cnt,
                                              uint64_t &e, uint64_t &d, uint32_t &p)
{
    const LvGeom &G = L.G;
    e = 0;
    d = 0;
    p = 0;
    if (G.nsub <= 64) { /* a lane per window */
        if (lane < cnt) {
            uint32_t lo, hi;
            lv_slots_of(G, L.k0 + m0 + lane, lo, hi);
            for (uint32_t j = lo; j < hi; j++) {
                const LvPart t = pc[j];
                e += t.energy;
                d += t.diff;
                p = t.peak > p ? t.peak : p;
            }
        }
    } else { /* long windows: the wave per window, lane j keeps window m0 + j */
        for (uint32_t j = 0; j < cnt; j++) {
            uint32_t lo, hi, wp;
            uint64_t we, wd;
            lv_slots_of(G, L.k0 + m0 + j, lo, hi);
            lv_wave_slots(pc, lane, lo, hi, we, wd, wp);
            if (lane == j) {
                e = we;
                d = wd;
                p = wp;
            }
        }
    }
    if (m0 + lane == 0) { /* what earlier calls left of the first window */
        e += s.energy;
        d += s.diff;
        p = s.peak > p ? s.peak : p;
    }
}

/* what the call leaves on the device: the unfinished window behind its completed ones, the last element and the squelch state.
 * The whole wave calls it; lane 0 stores. */
__device__ __forceinline__ void lv_leave(const LvFinish &L, const LvChan &s, const LvPart *pc, uint32_t lane, uint32_t c, uint32_t open, uint32_t bad)
{
    const LvGeom &G = L.G;
    uint64_t te = 0, td = 0;
    uint32_t tp = 0;
    if (L.tail) {
        uint32_t lo, hi;
        lv_slots_of(G, L.k0 + L.nwin, lo, hi);
        lv_wave_slots(pc, lane, lo, hi, te, td, tp);
    }
    if (lane == 0) {
        LvChan o;
        o.energy = te + (L.nwin ? 0ull : s.energy);
        o.diff = td + (L.nwin ? 0ull : s.diff);
        o.peak = L.nwin ? tp : (tp > s.peak ? tp : s.peak);
        o.prev = G.with_diff && G.N ? (uint32_t)(uint16_t)L.x[(size_t)c * L.stride + G.N - 1] : s.prev;
        o.open = open;
        o.bad = bad;
        L.st[c] = o;
        L.d_open[c] = open;
    }
}

} /* namespace mfm_lv */

/* mfm_level_adaptive.hip: queues lv_adaptive_finish_kernel, one wave per channel, in the place of lv_finish_kernel */
extern "C" __attribute__((visibility("hidden"))) int mfm_internal_level_adaptive_launch(const mfm_lv::LvFinish *finish,
                                                                                         const mfm_lv::LvAdaptive *adaptive,
                                                                                         uint32_t nr_channels, hipStream_t s);

#endif /* MFM_LEVEL_KERNELS_H */
