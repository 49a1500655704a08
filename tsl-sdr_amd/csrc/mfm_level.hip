/*
 * mfm_level.hip - per-channel signal level and squelch for all channels at once, on rows that are still in HBM: the
 * engine's PCM or filtered IQ, or the resampler's output.  See include/multifm_hip.h for the boundary and the record
 * format, mfm_level.h for the arithmetic.
 *
 * The reference has no such stage: an empty channel's discriminator noise runs through every decoder behind it.  What
 * the stage computes is defined exactly (integer sums over windows of W samples), so a numpy restatement is the
 * yardstick (tests/test_level.py).
 *
 * Layout of the work.  A row is a run of int16 ELEMENTS (one per sample in the PCM form, two in the IQ form); a window
 * is We = W or 2 W of them.  The stream of every channel is cut, in ABSOLUTE element positions, into SLOTS: window k
 * holds nsub = ceil(We / B) slots of B = min(We, 4096) elements (its last one may be shorter).  A slot never crosses
 * a window edge, so a partial sum belongs to one window; a call covers the slots that its elements [P, P + N) touch,
 * the first and last clipped to the call.
 *
 *   lv_wide_kernel    We >= 512: one WAVE per slot.  A lane takes 8 consecutive elements with one 16-byte load, a
 *                     wave 512 per step, 8 steps (a whole slot of 4096) are in flight together; the element in front
 *                     of a lane's first comes from its neighbour by one DPP move.  One wave reduction per slot.
 *   lv_narrow_kernel  We < 512: one LANE per slot (= per window), 16-byte loads along its own run.  A wave covers 64
 *                     consecutive windows, i.e. one contiguous piece of the row; what bounds it is the 40-byte record
 *                     per window, not the input.
 *   lv_finish_kernel  one wave per channel: adds the slots of every window the call completed (plus what earlier
 *                     calls left of the first one), writes the records, steps the squelch through them in stream
 *                     order and keeps the unfinished window's sums, the last element and the squelch state on the
 *                     device.
 *
 * With the adaptive squelch on (mfm_level_set_adaptive) lv_adaptive_finish_kernel (mfm_level_adaptive.hip, an object of its
 * own) is queued in the place of lv_finish_kernel; this file holds its setting and its two buffers.  What the two finish
 * kernels share is mfm_level_kernels.h.
 *
 * Nothing is floating point, no result goes through an atomic, and the host never waits: how many windows a call
 * completes follows from the stream position alone.
 */
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/multifm_hip.h"

#include "mfm_level.h"
#include "mfm_level_kernels.h"

extern "C" __attribute__((visibility("hidden"))) void mfm_internal_set_error(const char *msg);

namespace {

using namespace mfm_lv;

constexpr uint32_t LV_SLOT = 4096; /* elements per slot at most: 8 steps of 512 */
constexpr uint32_t LV_U = 8;       /* steps of one wave in flight */
constexpr uint32_t LV_NARROW = 512; /* windows below this many elements: a lane per window */

/* elements [a, b) of the call's rows that slot s of the call covers */
__device__ __forceinline__ void lv_slot_range(const LvGeom &G, uint32_t s, uint32_t &a, uint32_t &b)
{
    const uint64_t g = G.g0 + s;
    const uint64_t k = G.nsub == 1 ? g : g / G.nsub;
    const uint32_t q = (uint32_t)(g - k * G.nsub);
    const uint64_t st = k * G.We + (uint64_t)q * G.B;
    const uint64_t wend = (k + 1) * G.We;
    const uint64_t en = st + G.B < wend ? st + G.B : wend;
    const uint64_t lo = st > G.P ? st : G.P;
    const uint64_t hi = en < G.P + G.N ? en : G.P + G.N;
    a = (uint32_t)(lo - G.P);
    b = (uint32_t)(hi - G.P);
}

__global__ __launch_bounds__(256) void lv_wide_kernel(const LvGeom G, const int16_t *x, size_t stride, const LvChan *st, LvPart *parts,
                                                     uint32_t parts_stride)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t s = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    const uint32_t c = blockIdx.y;
    if (s >= G.nslots) {
        return;
    }
    uint32_t a, b;
    lv_slot_range(G, s, a, b);
    const int16_t *xc = x + (size_t)c * stride;
    const bool with_diff = G.with_diff != 0;
    /* the dword whose upper half is the element in front of the slot: the row's, or what the last call left */
    uint32_t last = 0;
    if (with_diff) {
        last = (a ? (uint32_t)(uint16_t)xc[a - 1] : st[c].prev) << 16;
    }
    mfm_level_acc acc{};
    for (uint32_t i0 = a; i0 < b; i0 += 512u * LV_U) {
        uint32_t d[LV_U][4];
#pragma unroll
        for (uint32_t u = 0; u < LV_U; u++) {
            const uint32_t i = i0 + 512u * u + 8u * lane;
            if (i + 8u <= b) {
                const mfm_level_x8 v = *reinterpret_cast<const mfm_level_x8 *>(xc + i);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    d[u][q] = v.d[q];
                }
            } else { /* the slot's end: element by element, zeros behind it */
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) {
                    const uint32_t e0 = i + 2u * q, e1 = e0 + 1u;
                    const uint32_t lo = e0 < b ? (uint16_t)xc[e0] : 0u;
                    const uint32_t hi = e1 < b ? (uint16_t)xc[e1] : 0u;
                    d[u][q] = lo | (hi << 16);
                }
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < LV_U; u++) {
            const uint32_t i = i0 + 512u * u + 8u * lane;
            const uint32_t valid = i >= b ? 0u : (b - i < 8u ? b - i : 8u);
            /* lane l takes lane l - 1's last dword (wave_shr:1), lane 0 the one of the step before */
            uint32_t up = 0;
            if (with_diff) {
                up = (uint32_t)__builtin_amdgcn_update_dpp((int)last, (int)d[u][3], 0x138, 0xf, 0xf, false);
                last = (uint32_t)__builtin_amdgcn_readlane((int)d[u][3], 63);
            }
            mfm_level_step8(acc, d[u], up, valid, with_diff);
        }
    }
    const uint64_t e = lv_wave_sum(acc.energy);
    const uint64_t df = with_diff ? lv_wave_sum(acc.diff) : 0ull;
    const uint32_t pk = lv_wave_max(mfm_level_peak(acc));
    if (lane == 0) {
        parts[(size_t)c * parts_stride + s] = LvPart{ e, df, pk, 0u };
    }
}

__global__ __launch_bounds__(256) void lv_narrow_kernel(const LvGeom G, const int16_t *x, size_t stride, const LvChan *st, LvPart *parts,
                                                       uint32_t parts_stride)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t c = blockIdx.y;
    if (s >= G.nslots) {
        return;
    }
    uint32_t a, b;
    lv_slot_range(G, s, a, b);
    const int16_t *xc = x + (size_t)c * stride;
    const bool with_diff = G.with_diff != 0;
    int16_t prev = 0;
    if (with_diff) {
        prev = a ? xc[a - 1] : (int16_t)(uint16_t)st[c].prev;
    }
    mfm_level_acc acc{};
    mfm_level_window(acc, xc + a, b - a, prev, with_diff);
    parts[(size_t)c * parts_stride + s] = LvPart{ acc.energy, acc.diff, mfm_level_peak(acc), 0u };
}

__global__ __launch_bounds__(64) void lv_finish_kernel(const LvFinish L)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t c = blockIdx.x;
    const LvChan s = L.st[c];
    const LvPart *pc = L.parts + (size_t)c * L.parts_stride;
    uint32_t open = s.open, bad = s.bad;
    mfm_level_record *rc = L.rec + (size_t)c * L.rec_stride;
    for (uint32_t m0 = 0; m0 < L.nwin; m0 += 64) {
        const uint32_t m = m0 + lane;
        const uint32_t cnt = L.nwin - m0 < 64u ? L.nwin - m0 : 64u;
        const bool act = lane < cnt;
        uint64_t e, d;
        uint32_t p;
        lv_round_sums(L, s, pc, lane, m0, cnt, e, d, p);
        const uint64_t metric = L.Q.use_diff ? d : e;
        uint32_t my_open = 0;
        const int mlo = (int)(uint32_t)metric, mhi = (int)(uint32_t)(metric >> 32);
        for (uint32_t j = 0; j < cnt; j++) { /* the squelch is sequential: the wave steps it as one (j is uniform: two lane reads
                                                 into scalar registers, scalar compares), lane j keeps step j */
            const uint64_t mj = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(mhi, (int)j) << 32) | (uint32_t)__builtin_amdgcn_readlane(mlo, (int)j);
            mfm_level_squelch_step(open, bad, L.Q.below, L.Q.open_thr, L.Q.close_thr, L.Q.hang, mj);
            if (lane == j) {
                my_open = open;
            }
        }
        if (act) {
            mfm_level_record r;
            r.energy = e;
            r.diff_energy = d;
            r.window = L.k0 + m;
            r.peak = p;
            r.channel = c;
            r.open = my_open;
            r.reserved = 0;
            rc[m] = r;
        }
    }
    lv_leave(L, s, pc, lane, c, open, bad); /* the unfinished window behind them, the last element, the squelch state */
}

thread_local char g_lv_error[256] = "";

int lv_inval(const char *msg)
{
    snprintf(g_lv_error, sizeof(g_lv_error), "%s", msg);
    mfm_internal_set_error(g_lv_error);
    return MFM_E_INVAL;
}

} /* namespace */

#define LV_TRY(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t err_ = (expr);                                                                            \
        if (err_ != hipSuccess) {                                                                            \
            snprintf(g_lv_error, sizeof(g_lv_error), "%s failed: %s", #expr, hipGetErrorString(err_));       \
            mfm_internal_set_error(g_lv_error);                                                              \
            return err_ == hipErrorOutOfMemory ? MFM_E_NOMEM : MFM_E_DEVICE;                                 \
        }                                                                                                    \
    } while (0)

struct mfm_level {
    mfm_level_config cfg{};
    uint32_t E = 1;          /* elements per sample */
    uint32_t We = 0, B = 0, nsub = 0;
    uint32_t max_win = 0;    /* records per channel and call at most */
    uint32_t max_slots = 0;
    uint64_t pos = 0;        /* samples per channel consumed so far */
    uint32_t last_nwin = 0;
    LvChan *d_st = nullptr;
    LvPart *d_parts = nullptr;
    mfm_level_record *d_rec = nullptr;
    uint32_t *d_open = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_call = false;
    /* the adaptive squelch (mfm_level_set_adaptive) */
    bool fresh = true;        /* no process call since create or the last seek */
    uint64_t fresh_pos = 0;   /* where create or the last seek put the stream: the floor looks no further back */
    bool adaptive = false;
    mfm_level_adaptive ad{};
    uint64_t *d_hist = nullptr;  /* [channel][max(M - 1, 1)] */
    uint64_t *d_floor = nullptr; /* [channel][max_win] */
};

extern "C" {

int mfm_level_create(struct mfm_level **pp, const struct mfm_level_config *cfg)
{
    if (!pp || !cfg) {
        return MFM_E_INVAL;
    }
    *pp = nullptr;
    if (cfg->abi_version != MFM_ABI_VERSION || 0 == cfg->nr_channels || cfg->nr_channels > 65535u || 0 == cfg->max_in_samples ||
        cfg->max_in_samples > (1u << 28) || cfg->flags != 0) {
        return lv_inval("abi_version, nr_channels (1 .. 65535), max_in_samples (1 .. 2^28) or flags (0) out of range");
    }
    if (0 == cfg->window_samples || cfg->window_samples > (1u << 30)) {
        return lv_inval("window_samples must be 1 .. 2^30");
    }
    if (cfg->form != MFM_LEVEL_PCM && cfg->form != MFM_LEVEL_IQ) {
        return lv_inval("form must be MFM_LEVEL_PCM or MFM_LEVEL_IQ");
    }
    if (cfg->metric != MFM_LEVEL_METRIC_ENERGY && cfg->metric != MFM_LEVEL_METRIC_DIFF) {
        return lv_inval("metric must be MFM_LEVEL_METRIC_ENERGY or MFM_LEVEL_METRIC_DIFF");
    }
    if (cfg->metric == MFM_LEVEL_METRIC_DIFF && cfg->form == MFM_LEVEL_IQ) {
        return lv_inval("the IQ form has no diff_energy to squelch on");
    }
    if (cfg->sense != MFM_LEVEL_OPEN_ABOVE && cfg->sense != MFM_LEVEL_OPEN_BELOW) {
        return lv_inval("sense must be MFM_LEVEL_OPEN_ABOVE or MFM_LEVEL_OPEN_BELOW");
    }
    if (cfg->sense == MFM_LEVEL_OPEN_ABOVE ? cfg->close_thr > cfg->open_thr : cfg->close_thr < cfg->open_thr) {
        return lv_inval("thresholds in the wrong order: close_thr <= open_thr for OPEN_ABOVE, close_thr >= open_thr for OPEN_BELOW");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) {
        return MFM_E_DEVICE; /* no CPU path */
    }
    LV_TRY(hipSetDevice(cfg->device));
    mfm_level *p = new (std::nothrow) mfm_level();
    if (!p) {
        return MFM_E_NOMEM;
    }
    p->cfg = *cfg;
    p->E = cfg->form == MFM_LEVEL_IQ ? 2u : 1u;
    p->We = cfg->window_samples * p->E;
    p->B = p->We < LV_SLOT ? p->We : LV_SLOT;
    p->nsub = (p->We + p->B - 1) / p->B;
    p->max_win = cfg->max_in_samples / cfg->window_samples + 1;
    /* whole slots of the call, one cut short per window edge, the clipped first and last */
    p->max_slots = (uint32_t)(((uint64_t)cfg->max_in_samples * p->E) / p->B) + p->max_win + 2;
    const uint32_t C = cfg->nr_channels;
    *pp = p;
    LV_TRY(hipMalloc(&p->d_st, (size_t)C * sizeof(LvChan)));
    LV_TRY(hipMemset(p->d_st, 0, (size_t)C * sizeof(LvChan))); /* nothing summed, x[-1] = 0, closed */
    LV_TRY(hipMalloc(&p->d_parts, (size_t)C * p->max_slots * sizeof(LvPart)));
    LV_TRY(hipMalloc(&p->d_rec, (size_t)C * p->max_win * sizeof(mfm_level_record)));
    LV_TRY(hipMalloc(&p->d_open, (size_t)C * 4));
    LV_TRY(hipMemset(p->d_open, 0, (size_t)C * 4));
    LV_TRY(hipDeviceSynchronize());
    return MFM_OK;
}

void mfm_level_destroy(struct mfm_level **pp)
{
    if (!pp || !*pp) {
        return;
    }
    mfm_level *p = *pp;
    (void)hipSetDevice(p->cfg.device);
    (void)hipDeviceSynchronize();
    (void)hipFree(p->d_st);
    (void)hipFree(p->d_parts);
    (void)hipFree(p->d_rec);
    (void)hipFree(p->d_open);
    (void)hipFree(p->d_hist);
    (void)hipFree(p->d_floor);
    delete p;
    *pp = nullptr;
}

int mfm_level_process_device(struct mfm_level *p, const int16_t *d_rows, size_t in_stride, size_t nr_in, void *stream)
{
    if (!p || (!d_rows && nr_in) || nr_in > p->cfg.max_in_samples || (nr_in && in_stride < nr_in * p->E && p->cfg.nr_channels > 1)) {
        return MFM_E_INVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    LV_TRY(hipSetDevice(p->cfg.device));
    if (p->have_call && p->last_stream != s) {
        LV_TRY(hipStreamSynchronize(p->last_stream)); /* state lives on the device; keep calls ordered */
    }
    const uint32_t C = p->cfg.nr_channels, W = p->cfg.window_samples;
    const uint64_t k0 = p->pos / W, k1 = (p->pos + nr_in) / W;
    const uint32_t nwin = (uint32_t)(k1 - k0);
    if (nr_in) {
        LvGeom G{};
        G.P = p->pos * p->E;
        G.N = (uint32_t)nr_in * p->E;
        G.We = p->We;
        G.B = p->B;
        G.nsub = p->nsub;
        G.with_diff = p->cfg.form == MFM_LEVEL_PCM;
        const uint64_t last = G.P + G.N - 1;
        G.g0 = k0 * G.nsub + (G.P - k0 * G.We) / G.B;
        const uint64_t kl = last / G.We;
        const uint64_t g1 = kl * G.nsub + (last - kl * G.We) / G.B;
        G.nslots = (uint32_t)(g1 - G.g0 + 1);
        if (G.nslots > p->max_slots || nwin > p->max_win) {
            return lv_inval("internal: slot count exceeds the plan");
        }
        if (G.We >= LV_NARROW) {
            hipLaunchKernelGGL(lv_wide_kernel, dim3((G.nslots + 3) / 4, C), dim3(256), 0, s, G, d_rows, in_stride, p->d_st, p->d_parts,
                               p->max_slots);
        } else {
            hipLaunchKernelGGL(lv_narrow_kernel, dim3((G.nslots + 255) / 256, C), dim3(256), 0, s, G, d_rows, in_stride, p->d_st,
                               p->d_parts, p->max_slots);
        }
        LV_TRY(hipGetLastError());
        LvFinish F{};
        F.G = G;
        F.Q = LvSquelch{ p->cfg.open_thr, p->cfg.close_thr, p->cfg.metric == MFM_LEVEL_METRIC_DIFF ? 1u : 0u,
                         p->cfg.sense == MFM_LEVEL_OPEN_BELOW ? 1u : 0u, p->cfg.hang_windows, 0u };
        F.x = d_rows;
        F.stride = in_stride;
        F.st = p->d_st;
        F.parts = p->d_parts;
        F.parts_stride = p->max_slots;
        F.rec = p->d_rec;
        F.rec_stride = p->max_win;
        F.d_open = p->d_open;
        F.k0 = k0;
        F.nwin = nwin;
        F.tail = (p->pos + nr_in) % W ? 1u : 0u;
        if (p->adaptive) { /* the same two input kernels, the adaptive finish kernel (mfm_level_adaptive.hip) behind them */
            LvAdaptive A{};
            A.M = p->ad.floor_windows;
            A.open_q8 = p->ad.open_q8;
            A.close_q8 = p->ad.close_q8;
            A.warmup = p->ad.warmup_windows;
            A.done = k0 - p->fresh_pos / W;
            A.hist = p->d_hist;
            A.hist_stride = A.M > 1 ? A.M - 1 : 1;
            A.floor = p->d_floor;
            A.floor_stride = p->max_win;
            if (mfm_internal_level_adaptive_launch(&F, &A, C, s) != MFM_OK) {
                return lv_inval("internal: the adaptive finish kernel was not queued");
            }
        } else {
            hipLaunchKernelGGL(lv_finish_kernel, dim3(C), dim3(64), 0, s, F);
        }
        LV_TRY(hipGetLastError());
    }
    p->fresh = false;
    p->pos += nr_in;
    p->last_nwin = nwin;
    p->last_stream = s;
    p->have_call = true;
    return MFM_OK;
}

int mfm_level_process_host(struct mfm_level *p, const int16_t *rows, size_t in_stride, size_t nr_in)
{
    if (!p || (!rows && nr_in)) {
        return MFM_E_INVAL;
    }
    LV_TRY(hipSetDevice(p->cfg.device));
    const uint32_t C = p->cfg.nr_channels;
    const size_t ne = nr_in * p->E;
    int16_t *d_in = nullptr;
    LV_TRY(hipMalloc(&d_in, (size_t)C * (ne ? ne : 1) * 2));
    if (ne) {
        LV_TRY(hipMemcpy2D(d_in, ne * 2, rows, in_stride * 2, ne * 2, C, hipMemcpyHostToDevice));
    }
    const int rc = mfm_level_process_device(p, d_in, ne, nr_in, nullptr);
    (void)hipDeviceSynchronize();
    (void)hipFree(d_in);
    return rc;
}

int mfm_level_seek(struct mfm_level *p, uint64_t samples_before)
{
    if (!p) {
        return lv_inval("mfm_level_seek: no object");
    }
    if (samples_before >= (1ull << 62)) {
        return lv_inval("mfm_level_seek: samples_before must stay below 2^62");
    }
    if (samples_before % p->cfg.window_samples) {
        return lv_inval("mfm_level_seek: samples_before must be a multiple of window_samples (no fresh stage stands inside a window)");
    }
    LV_TRY(hipSetDevice(p->cfg.device));
    if (p->have_call) {
        LV_TRY(hipStreamSynchronize(p->last_stream));
    }
    const uint32_t C = p->cfg.nr_channels;
    LV_TRY(hipMemset(p->d_st, 0, (size_t)C * sizeof(LvChan))); /* as create: nothing summed, x[-1] = 0, closed */
    LV_TRY(hipMemset(p->d_open, 0, (size_t)C * 4));
    LV_TRY(hipDeviceSynchronize());
    p->pos = samples_before;
    p->last_nwin = 0;
    p->last_stream = nullptr;
    p->have_call = false;
    p->fresh = true; /* the adaptive setting stays; its history and warm-up count start over, both follow from fresh_pos */
    p->fresh_pos = samples_before;
    return MFM_OK;
}

int mfm_level_set_adaptive(struct mfm_level *p, const struct mfm_level_adaptive *a)
{
    if (!p) {
        return lv_inval("mfm_level_set_adaptive: no object");
    }
    if (!p->fresh) {
        return lv_inval("mfm_level_set_adaptive: only on a fresh object (after create or mfm_level_seek, before the next process call)");
    }
    if (a) {
        if (0 == a->floor_windows || a->floor_windows > 1024u) {
            return lv_inval("mfm_level_set_adaptive: floor_windows must be 1 .. 1024");
        }
        if (0 == a->open_q8 || a->open_q8 > 65536u || 0 == a->close_q8 || a->close_q8 > 65536u) {
            return lv_inval("mfm_level_set_adaptive: open_q8 and close_q8 must be 1 .. 65536");
        }
        if (p->cfg.sense == MFM_LEVEL_OPEN_ABOVE ? a->close_q8 > a->open_q8 : a->close_q8 < a->open_q8) {
            return lv_inval("mfm_level_set_adaptive: ratios in the wrong order: close_q8 <= open_q8 for OPEN_ABOVE, close_q8 >= open_q8 for OPEN_BELOW");
        }
        if (a->flags != 0 || a->reserved != 0) {
            return lv_inval("mfm_level_set_adaptive: flags and reserved must be 0");
        }
    }
    LV_TRY(hipSetDevice(p->cfg.device));
    if (!a) {
        p->adaptive = false;
        return MFM_OK;
    }
    const uint32_t C = p->cfg.nr_channels;
    const size_t hist = a->floor_windows > 1 ? a->floor_windows - 1 : 1;
    uint64_t *d_hist = nullptr, *d_floor = nullptr;
    if (hipMalloc(&d_hist, (size_t)C * hist * 8) != hipSuccess || hipMalloc(&d_floor, (size_t)C * p->max_win * 8) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(d_hist);
        return MFM_E_NOMEM; /* the object is as it was */
    }
    (void)hipFree(p->d_hist); /* fresh: nothing queued reads them */
    (void)hipFree(p->d_floor);
    p->d_hist = d_hist;
    p->d_floor = d_floor;
    p->ad = *a;
    p->adaptive = true;
    return MFM_OK;
}

int mfm_level_get_adaptive(struct mfm_level *p, uint32_t *on, struct mfm_level_adaptive *a)
{
    if (!p) {
        return MFM_E_INVAL;
    }
    if (on) {
        *on = p->adaptive ? 1u : 0u;
    }
    if (a) {
        *a = p->adaptive ? p->ad : mfm_level_adaptive{};
    }
    return MFM_OK;
}

int mfm_level_fetch_floor(struct mfm_level *p, uint64_t *out, size_t max_values, size_t *nr_windows)
{
    if (!p || !nr_windows || (!out && max_values)) {
        return MFM_E_INVAL;
    }
    if (!p->adaptive) {
        return lv_inval("mfm_level_fetch_floor: the adaptive squelch is off");
    }
    *nr_windows = p->last_nwin;
    if (!p->have_call || 0 == p->last_nwin) {
        return MFM_OK;
    }
    const uint32_t C = p->cfg.nr_channels;
    if ((size_t)C * p->last_nwin > max_values) {
        return MFM_E_NOMEM;
    }
    LV_TRY(hipSetDevice(p->cfg.device));
    LV_TRY(hipStreamSynchronize(p->last_stream));
    const size_t row = (size_t)p->last_nwin * 8;
    LV_TRY(hipMemcpy2D(out, row, p->d_floor, (size_t)p->max_win * 8, row, C, hipMemcpyDeviceToHost));
    return MFM_OK;
}

int mfm_level_floor_view(struct mfm_level *p, const uint64_t **d_floor, size_t *floor_stride)
{
    if (!p) {
        return MFM_E_INVAL;
    }
    if (!p->adaptive) {
        return lv_inval("mfm_level_floor_view: the adaptive squelch is off");
    }
    if (d_floor) {
        *d_floor = p->d_floor;
    }
    if (floor_stride) {
        *floor_stride = p->max_win;
    }
    return MFM_OK;
}

int mfm_level_fetch(struct mfm_level *p, struct mfm_level_record *out, size_t max_records, size_t *nr_windows)
{
    if (!p || !nr_windows || (!out && max_records)) {
        return MFM_E_INVAL;
    }
    *nr_windows = p->last_nwin;
    if (!p->have_call || 0 == p->last_nwin) {
        return MFM_OK;
    }
    const uint32_t C = p->cfg.nr_channels;
    if ((size_t)C * p->last_nwin > max_records) {
        return MFM_E_NOMEM;
    }
    LV_TRY(hipSetDevice(p->cfg.device));
    LV_TRY(hipStreamSynchronize(p->last_stream));
    const size_t row = (size_t)p->last_nwin * sizeof(mfm_level_record);
    LV_TRY(hipMemcpy2D(out, row, p->d_rec, (size_t)p->max_win * sizeof(mfm_level_record), row, C, hipMemcpyDeviceToHost));
    return MFM_OK;
}

int mfm_level_device_view(struct mfm_level *p, const struct mfm_level_record **d_records, size_t *record_stride, size_t *nr_windows,
                          const uint32_t **d_open)
{
    if (!p) {
        return MFM_E_INVAL;
    }
    if (d_records) {
        *d_records = p->d_rec;
    }
    if (record_stride) {
        *record_stride = p->max_win;
    }
    if (nr_windows) {
        *nr_windows = p->last_nwin;
    }
    if (d_open) {
        *d_open = p->d_open;
    }
    return MFM_OK;
}

void mfm_hosttwin_level_window(const int16_t *x, size_t nr_samples, uint32_t form, int16_t prev, uint64_t *energy, uint64_t *diff_energy,
                               uint32_t *peak)
{
    mfm_level_acc acc{};
    const bool pcm = form == MFM_LEVEL_PCM;
    if (x && nr_samples) {
        mfm_level_window(acc, x, (uint32_t)(nr_samples * (pcm ? 1u : 2u)), prev, pcm);
    }
    if (energy) {
        *energy = acc.energy;
    }
    if (diff_energy) {
        *diff_energy = acc.diff;
    }
    if (peak) {
        *peak = mfm_level_peak(acc);
    }
}

uint32_t mfm_hosttwin_squelch_step(uint32_t sense, uint64_t open_thr, uint64_t close_thr, uint32_t hang_windows, uint64_t metric,
                                   uint32_t *open, uint32_t *bad)
{
    if (!open || !bad) {
        return 0;
    }
    mfm_level_squelch_step(*open, *bad, sense == MFM_LEVEL_OPEN_BELOW ? 1u : 0u, open_thr, close_thr, hang_windows, metric);
    return *open;
}

void mfm_hosttwin_level_adaptive(const uint64_t *metric, size_t nr_windows, uint32_t sense, uint64_t open_thr, uint64_t close_thr,
                                 uint32_t hang_windows, const struct mfm_level_adaptive *a, uint64_t *floor, uint32_t *open)
{
    if (!metric || !a || 0 == a->floor_windows) {
        return;
    }
    const uint32_t below = sense == MFM_LEVEL_OPEN_BELOW ? 1u : 0u;
    uint32_t op = 0, bad = 0;
    for (size_t k = 0; k < nr_windows; k++) {
        const size_t first = k + 1 > a->floor_windows ? k + 1 - a->floor_windows : 0;
        uint64_t key = ~0ull; /* the sliding minimum of the keys, window by window: the definition, not the kernel's doubling */
        for (size_t j = first; j <= k; j++) {
            const uint64_t kj = mfm_level_floor_key(below, metric[j]);
            key = kj < key ? kj : key;
        }
        const uint64_t f = mfm_level_floor_key(below, key);
        bool on_open_side, is_bad;
        mfm_level_adaptive_predicates(below, metric[k], f, a->open_q8, a->close_q8, open_thr, close_thr, k < a->warmup_windows, on_open_side,
                                      is_bad);
        mfm_level_squelch_step_bits(op, bad, hang_windows, on_open_side, is_bad);
        if (floor) {
            floor[k] = f;
        }
        if (open) {
            open[k] = op;
        }
    }
}

} /* extern "C" */
