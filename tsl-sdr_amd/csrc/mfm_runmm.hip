/*
 * mfm_runmm.hip - the burst Mueller-Muller stage: the runs the burst resampler left in its dense payload go through the clock
 * recovery loop (pager/mueller_muller.c:10-115) on the device, one fresh loop per stretch.  See include/multifm_hip.h for the
 * boundary and the result, mfm_runmm.h for the position, the slot bound and the arithmetic of a decision, mfm_run_stage.h for
 * the checks of a run, and mfm_mm.hip for the row stage whose walk this file restates.
 *
 * The input is what mfm_runrs_device_view returns; how many runs and samples a call carries is read on the device, so the
 * host never waits and every launch is sized from the capacities fixed at create.
 *
 *   rm_plan_kernel     one block.  One pass over the runs: every run is checked (mfm_run_check_run) before anything of the
 *                      payload is read; exclusive scan of the runs' decision slots; a channel's last run leaves its index for
 *                      the state kernel; the totals and the flags.
 *   rm_walk_kernel     The loop is a feedback loop: the time of a run is the length of its dependent chain, and the runs of a
 *                      call are independent chains, so the parallelism is the number of runs.  One lane per run, RM_RUNS = 16 runs
 *                      per one-wave workgroup, as mfm_mm_kernel takes 16 rows: the chain costs a wave the same time whether 16 or
 *                      64 of its lanes walk, while the staging it does grows with the runs.  Each run has a strip of RM_U = 512
 *                      samples in LDS, and the whole wave stages: a run's next unit is one instruction of 64 lanes on 1 KB of
 *                      consecutive memory, 16-byte loads on the 16-byte grid of the payload (out_offset has any 2-byte alignment),
 *                      requested into registers before the current units are walked and written to the strips behind the walk;
 *                      the samples in front of the grid and behind a run's last whole group go singly, by the run's own lane.
 *                      The walk is mfm_mm_kernel's: the four samples the next decision can fall on are read from the strip as one
 *                      8-byte word as soon as the index of this one is known, and the one it did fall on is shifted out when the
 *                      step is, so the float arithmetic alone is the dependent chain.  Decisions go to the run's slot range; the
 *                      run's record and the state it ends in are left per run.  A wave runs as long as its longest run.
 *   rm_scan_kernel     one block: exclusive scan of the runs' decision counts into dec_offset, the total.
 *   rm_compact_kernel  one wave per run: its decisions from the slot range into the dense payload.
 *   rm_state_kernel    one lane per channel: the state of the channel's last run goes into the OTHER of two state buffers; a
 *                      channel without a run, and every channel of a refused call, copies its state over.
 *
 * No atomic decides a placement and nothing is read behind a run.  The block scan, a thread's slice of the runs, the plan's
 * head and the host code around a call are mfm_run_stage.h's, shared with the other burst stages.
 */
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/multifm_hip.h"

#include "mfm_runmm.h"

static_assert(sizeof(mfm_runmm_run) == 40 && offsetof(mfm_runmm_run, first_dec) == 16 && offsetof(mfm_runmm_run, channel) == 24,
              "struct mfm_runmm_run is 40 bytes");
static_assert(sizeof(mfm_runmm_state) == 48 && offsetof(mfm_runmm_state, w) == 24 && offsetof(mfm_runmm_state, next_offset) == 36,
              "struct mfm_runmm_state is 48 bytes");

namespace {

constexpr uint32_t RM_T_RUNS = 0, RM_T_DECS = 1; /* d_totals[], in front of MFM_RUN_T_OVERFLOW and MFM_RUN_T_INPUT */
constexpr uint32_t RM_RUNS = 16;                  /* runs (walking lanes) per one-wave workgroup */
constexpr uint32_t RM_U = MFM_RUNMM_STAGING_UNIT; /* samples of a run in its strip: the walk's staging unit */
constexpr uint32_t RM_PITCH = RM_U * 2u + 16u;    /* bytes per strip: the 8-byte candidate read may start at the last sample */
static_assert(RM_U == 64u * 8u, "a unit is one 16-byte group per lane of the wave");
static_assert((RM_RUNS & (RM_RUNS - 1u)) == 0, "a lane's strip is picked with a mask");

typedef uint32_t rm_u32x4 __attribute__((ext_vector_type(4))); /* (HIP's uint4 is a struct of unions: arrays of it end up in scratch) */
typedef rm_u32x4 __attribute__((may_alias)) rm_u32x4_a;
typedef int16_t __attribute__((may_alias)) rm_i16_a;

struct RmCall {
    const mfm_runrs_run *runs;
    const int16_t *payload;
    const uint64_t *rtotals;
    const mfm_runmm_state *chan_old;
    mfm_runmm_state *chan_new;
    mfm_runmm_state *run_state; /* [cap_runs] what a run's walk ends in */
    mfm_runmm_run *out_runs;    /* [cap_runs] */
    uint32_t *slot_base;        /* [cap_runs] first decision slot of a run */
    uint32_t *chan_last;        /* [C] */
    uint32_t *ctl;              /* [0] runs, 0 for a refused call */
    uint64_t *totals;
    int16_t *slots;             /* [cap_decs] */
    int16_t *decs;              /* [cap_decs] */
    uint32_t C, cap_runs, cap_out, cap_decs;
    mfm_runmm_params P;
};

__global__ __launch_bounds__(MFM_RUN_SCAN_THREADS) void rm_plan_kernel(const RmCall A)
{
    __shared__ uint64_t lds[MFM_RUN_SCAN_THREADS / 64];
    uint64_t n, E, over, err, r0, r1;
    if (!mfm_run_plan_head(A.rtotals, A.cap_out, A.cap_runs, A.totals, A.ctl, 1, &n, &E, &over, &err)) {
        return; /* nothing may be read */
    }
    mfm_run_slice(n, &r0, &r1);
    uint64_t so = 0, ss = 0;
    uint32_t bad = 0;
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) {
        const mfm_runrs_run run = A.runs[r];
        bad |= mfm_run_check_run(run, r ? &A.runs[r - 1] : nullptr, A.C, E, A.chan_old);
        so += run.nr_out;
        ss += mfm_runmm_slots(run.nr_out, A.P.s);
    }
    /* fewer than 2^28 runs of fewer than 2^32 outputs: every sum stays below 2^63 */
    uint64_t to, ts;
    (void)mfm_run_block_scan(so, lds, &to);
    uint64_t bs = mfm_run_block_scan(ss, lds, &ts);
    if (__syncthreads_or((bad & MFM_RUNMM_IN_OUT_OF_STEP) != 0)) {
        err |= MFM_RUNMM_IN_OUT_OF_STEP;
    }
    /* ranges that overlap could ask for more than the payload holds */
    if (__syncthreads_or((bad & MFM_RUNMM_IN_BAD_RUNS) != 0) || to > A.cap_out) {
        err |= MFM_RUNMM_IN_BAD_RUNS;
    }
    if (!err && ts > A.cap_decs) {
        over = MFM_RUNMM_OVER_DECISIONS;
    }
    const bool refused = over || err;
    if (!refused) { /* within the capacities: the slots fit 32 bits (rm_geometry) */
#pragma unroll 1
        for (uint64_t r = r0; r < r1; r++) {
            const uint32_t nr_out = A.runs[r].nr_out, c = A.runs[r].channel;
            A.slot_base[r] = (uint32_t)bs;
            bs += mfm_runmm_slots(nr_out, A.P.s);
            if (r + 1 == n || A.runs[r + 1].channel != c) {
                A.chan_last[c] = (uint32_t)r;
            }
        }
    }
    if (threadIdx.x == 0) {
        A.totals[RM_T_RUNS] = refused ? 0u : n;
        A.totals[RM_T_DECS] = 0; /* the decision scan */
        A.totals[MFM_RUN_T_OVERFLOW] = over;
        A.totals[MFM_RUN_T_INPUT] = err;
        A.ctl[0] = refused ? 0u : (uint32_t)n;
    }
}

__global__ __launch_bounds__(64) void rm_walk_kernel(const RmCall A)
{
    __shared__ __attribute__((aligned(16))) unsigned char strips[RM_RUNS * RM_PITCH];
    const uint32_t lane = threadIdx.x;
    const uint32_t n_runs = A.ctl[0]; /* 0 for a refused call */
    if (blockIdx.x * RM_RUNS >= n_runs) { /* surplus waves: the launch is sized from the capacity */
        return;
    }
    const uint32_t r = blockIdx.x * RM_RUNS + lane;
    const bool live = lane < RM_RUNS && r < n_runs;
    mfm_runrs_run run;
    if (live) {
        run = A.runs[r];
    } else { /* a lane without a run walks nothing and has nothing staged */
        run.first_window = run.out_offset = run.first_out = 0;
        run.channel = run.nr_out = run.reserved = 0;
        run.flags = MFM_RUNRS_BEGINS;
    }
    const mfm_runmm_params P = A.P;
    mfm_runmm_state st = mfm_runmm_start(A.chan_old[run.channel], run, P.spb);
    const uint32_t n = run.nr_out;
    const int16_t *p = A.payload + run.out_offset; /* [out_offset, out_offset + nr_out) lies within the totals (the plan) */
    /* strip coordinates: sample j of the run is q = a + j, so that the 16-byte groups of the strip are those of the memory */
    const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(p) >> 1) & 7u;
    const uint32_t qend = a + n;
    const uint32_t smin = P.s - 1u; /* the candidates: steps of s - 1 .. s + 2 (one below the shortest, as mfm_mm_kernel) */
    unsigned char *my = strips + (lane & (RM_RUNS - 1u)) * RM_PITCH;
    int16_t *dec = A.slots + (live ? A.slot_base[r] : 0u);
    const uint32_t cap = mfm_runmm_slots(n, P.s);
    uint32_t q = a + st.next_offset; /* below 2^31 + 2^21 + 8 */
    uint32_t kc = q / RM_U;          /* the unit the run's strip holds */
    uint32_t n_dec = 0;
    mfm_runmm_carry k{ st.w, st.m, st.last_sample, mfm_runmm_sign(st.last_sample) };
    rm_u32x4 v[RM_RUNS];
    bool act = q < qend;

    /* Staging is the whole wave's: group `lane` (8 samples) of a unit of every run i of the wave, a run's unit being one
     * instruction of 64 lanes on 1 KB of consecutive memory.  What a lane needs of run i it reads from i's lane once: g[i], its
     * group of the run's unit counted in 16-byte groups from the payload's grid, and rem[i], the samples from that group's
     * first to the run's end (0 when there are none): the group lies wholly inside the run where rem[i] >= 8, but for the first
     * group of a run that begins inside it (head, unit 0 alone).  From unit to unit g goes on by 64 and rem down by RM_U. */
    /* the payload rounded down to its 16-byte grid, by byte arithmetic on the kernel's own pointer: an address made from an integer
     * loses its address space and is loaded by flat_load, which counts on lgkmcnt as well and would be waited for with the strips */
    const unsigned char *gridp = reinterpret_cast<const unsigned char *>(A.payload) - (reinterpret_cast<uintptr_t>(A.payload) & 15u);
    const uint64_t grid = reinterpret_cast<uintptr_t>(A.payload) & ~(uint64_t)15u;
    uint32_t g[RM_RUNS], rem[RM_RUNS], head = 0;
#pragma unroll
    for (uint32_t i = 0; i < RM_RUNS; i++) {
        const uint32_t ai = (uint32_t)__builtin_amdgcn_readlane((int)a, (int)i), qe = (uint32_t)__builtin_amdgcn_readlane((int)qend, (int)i);
        const uint32_t ui = (uint32_t)__builtin_amdgcn_readlane((int)kc, (int)i);
        const uint64_t pa = reinterpret_cast<uintptr_t>(p);
        const uint64_t pi = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(pa >> 32), (int)i) << 32) |
                            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)pa, (int)i);
        const uint64_t q0 = (uint64_t)ui * RM_U + lane * 8u;
        g[i] = (uint32_t)((pi - 2u * ai - grid) >> 4) + ui * (RM_U / 8u) + lane; /* the payload has fewer than 2^28 groups */
        rem[i] = qe > q0 ? (uint32_t)(qe - q0) : 0u;
        head |= (ui == 0u && ai != 0u && lane == 0u ? 1u : 0u) << i;
    }
    /* the whole groups of the runs' next units into registers */
    auto fetch = [&](uint32_t first) {
#pragma unroll
        for (uint32_t i = 0; i < RM_RUNS; i++) {
            rm_u32x4 t = { 0u, 0u, 0u, 0u };
            if (rem[i] >= 8u && !(first & (head >> i) & 1u)) {
                t = *reinterpret_cast<const rm_u32x4_a *>(gridp + (size_t)g[i] * 16u);
            }
            v[i] = t;
        }
    };
    /* ... and into the strips, unit u of this lane's own run with them: what the run holds in front of the grid and behind its
     * last whole group */
    auto commit = [&](uint32_t first, uint32_t u) {
#pragma unroll
        for (uint32_t i = 0; i < RM_RUNS; i++) {
            if (rem[i] >= 8u && !(first & (head >> i) & 1u)) {
                *reinterpret_cast<rm_u32x4_a *>(strips + i * RM_PITCH + lane * 16u) = v[i];
            }
            rem[i] = rem[i] >= RM_U ? rem[i] - RM_U : 0u;
            g[i] += RM_U / 8u;
        }
        if (act && u == 0u && a != 0u) {
            const uint32_t he = qend < 8u ? qend : 8u;
            for (uint32_t qq = a; qq < he; qq++) {
                *reinterpret_cast<rm_i16_a *>(my + qq * 2u) = p[qq - a];
            }
        }
        const uint32_t t0 = qend & ~7u;
        if (act && (qend & 7u) != 0u && !(t0 == 0u && a != 0u) && t0 / RM_U == u) {
            for (uint32_t qq = t0; qq < qend; qq++) {
                *reinterpret_cast<rm_i16_a *>(my + (qq & (RM_U - 1u)) * 2u) = p[qq - a];
            }
        }
    };

    fetch(1u);
    commit(1u, kc);
    while (__any(act)) {
        fetch(0u);       /* nothing where a run ends in this unit */
        __syncthreads(); /* one wave: the strips' writes before the walk's reads */
        if (act) {
            const uint32_t e = (kc + 1u) * RM_U;
            const uint32_t lim = e < qend ? e : qend;
            bool go = q < lim;
            int32_t raw = go ? (int32_t)*reinterpret_cast<const rm_i16_a *>(my + (q & (RM_U - 1u)) * 2u) : 0; /* :66 */
            while (go) {
                const uint32_t pb = q + smin;
                uint64_t cand;
                /* raw is waited for here, in front of the candidates' request: asked for behind it, the wait for raw (the
                 * counter knows no single read) would be a wait for the candidates as well, the strip's latency on the chain */
                asm volatile("" : "+v"(raw) : : "memory");
                __builtin_memcpy(&cand, my + (pb & (RM_U - 1u)) * 2u, 8);
                dec[n_dec < cap ? n_dec : cap - 1u] = (int16_t)raw; /* :71; always n_dec: the slot bound (mfm_runmm_slots), cap >= 1 */
                n_dec++;
                q += mfm_runmm_step(k, P, raw);
                go = q < lim;
                const uint32_t d = q - pb;
                raw = (int32_t)(int16_t)(cand >> ((d & 3u) * 16u));
                if (go && d > 3u) { /* a step outside the four: the first decisions of a stretch, an unsettled loop */
                    raw = (int32_t)*reinterpret_cast<const rm_i16_a *>(my + (q & (RM_U - 1u)) * 2u);
                }
            }
        }
        __syncthreads(); /* the walk's reads before the next unit's writes */
        /* the registers hold unit kc + 1 of every run; one that has ended walks no more (what is left of it is shorter than
         * its last step, and staging it does no harm) */
        act = act && (uint64_t)(kc + 1u) * RM_U < qend && q < qend;
        commit(0u, kc + 1u);
        kc++;
    }
    if (live) {
        n_dec = n_dec < cap ? n_dec : cap;
        mfm_runmm_run o;
        o.first_window = run.first_window;
        o.dec_offset = 0; /* the decision scan */
        o.first_dec = st.decs;
        o.channel = run.channel;
        o.nr_dec = n_dec;
        o.flags = run.flags & MFM_RUNRS_BEGINS;
        o.reserved = 0;
        A.out_runs[r] = o;
        mfm_runmm_leave(st, k, q - a, n, n_dec);
        A.run_state[r] = st;
    }
}

__global__ __launch_bounds__(MFM_RUN_SCAN_THREADS) void rm_scan_kernel(const RmCall A)
{
    __shared__ uint64_t lds[MFM_RUN_SCAN_THREADS / 64];
    uint64_t r0, r1;
    mfm_run_slice<uint64_t>(A.ctl[0], &r0, &r1); /* 0 runs for a refused call */
    uint64_t s = 0;
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) {
        s += A.out_runs[r].nr_dec;
    }
    uint64_t total;
    uint64_t base = mfm_run_block_scan(s, lds, &total); /* at most the sum of the slots: within cap_decs */
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) {
        A.out_runs[r].dec_offset = base;
        base += A.out_runs[r].nr_dec;
    }
    if (threadIdx.x == 0) {
        A.totals[RM_T_DECS] = total;
    }
}

__global__ __launch_bounds__(64) void rm_compact_kernel(const RmCall A)
{
    const uint32_t r = blockIdx.x;
    if (r >= A.ctl[0]) {
        return;
    }
    const int16_t *src = A.slots + A.slot_base[r];
    int16_t *dst = A.decs + A.out_runs[r].dec_offset;
    const uint32_t nd = A.out_runs[r].nr_dec; /* at most the run's slots */
    for (uint32_t i = threadIdx.x; i < nd; i += blockDim.x) {
        dst[i] = src[i];
    }
}

__global__ __launch_bounds__(256) void rm_state_kernel(const RmCall A)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= A.C) {
        return;
    }
    const uint32_t last = A.chan_last[c];
    A.chan_last[c] = MFM_RUN_NONE; /* for the next call */
    const bool refused = A.totals[MFM_RUN_T_OVERFLOW] != 0 || A.totals[MFM_RUN_T_INPUT] != 0;
    A.chan_new[c] = last == MFM_RUN_NONE || refused ? A.chan_old[c] : A.run_state[last]; /* else the state stays */
}

/* what create checks without a device; the loop's constants and the decision capacity with the default filled in */
int rm_geometry(const mfm_runmm_config &cfg, mfm_runmm_params *P, uint64_t *cap_decs)
{
    const int rc = mfm_run_geometry(cfg);
    if (rc != MFM_OK) {
        return rc;
    }
    if (const char *why = mfm_runmm_params_check(cfg.kw, cfg.km, cfg.samples_per_bit, cfg.error_min, cfg.error_max, P)) {
        return mfm_run_fail(MFM_E_INVAL, why);
    }
    /* the sum of mfm_runmm_slots over max_runs runs that share max_out_samples outputs, at most */
    *cap_decs = cfg.max_decisions ? cfg.max_decisions : (uint64_t)cfg.max_out_samples / P->s + cfg.max_runs;
    return MFM_OK;
}

/* the message of a refused call, as fetch and the host twin give it */
const char *rm_refusal(uint64_t over, uint64_t err)
{
    return mfm_run_refusal(over, err, "the call's decision bound (the sum of nr_out / s + 1 over its runs, s = floor(error_min - |km| * 32768)) exceeds max_decisions");
}

} /* namespace */

struct mfm_runmm {
    mfm_runmm_config cfg{};
    mfm_runmm_params P{};
    uint64_t cap_decs = 0;
    mfm_runmm_state *d_chan[2] = { nullptr, nullptr }; /* used in turn: a call reads [cur] and writes [cur ^ 1] */
    uint32_t cur = 0;
    mfm_runmm_state *d_run_state = nullptr;
    mfm_runmm_run *d_out_runs = nullptr;
    uint32_t *d_slot_base = nullptr, *d_chan_last = nullptr, *d_ctl = nullptr;
    uint64_t *d_totals = nullptr;
    int16_t *d_slots = nullptr, *d_decs = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_call = false;
};

extern "C" {

int mfm_runmm_create(struct mfm_runmm **pm, const struct mfm_runmm_config *cfg)
{
    if (!pm || !cfg) {
        return MFM_E_INVAL;
    }
    *pm = nullptr;
    mfm_runmm_params P{};
    uint64_t cap_decs = 0;
    const int rc = rm_geometry(*cfg, &P, &cap_decs);
    if (rc != MFM_OK) {
        return rc;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) {
        return MFM_E_DEVICE; /* no CPU path */
    }
    mfm_runmm *m = new (std::nothrow) mfm_runmm();
    if (!m) {
        return MFM_E_NOMEM;
    }
    m->cfg = *cfg;
    m->P = P;
    m->cap_decs = cap_decs;
    const size_t C = cfg->nr_channels, nruns = cfg->max_runs;
    *pm = m; /* from here on the caller's destroy frees what was allocated */
    MFM_RUN_TRY(hipSetDevice(cfg->device));
    for (int i = 0; i < 2; i++) {
        MFM_RUN_TRY(hipMalloc(&m->d_chan[i], C * sizeof(mfm_runmm_state)));
        MFM_RUN_TRY(hipMemset(m->d_chan[i], 0, C * sizeof(mfm_runmm_state))); /* no stretch */
    }
    MFM_RUN_TRY(hipMalloc(&m->d_run_state, nruns * sizeof(mfm_runmm_state)));
    MFM_RUN_TRY(hipMalloc(&m->d_out_runs, nruns * sizeof(mfm_runmm_run)));
    MFM_RUN_TRY(hipMalloc(&m->d_slot_base, nruns * 4));
    MFM_RUN_TRY(hipMalloc(&m->d_chan_last, C * 4));
    MFM_RUN_TRY(hipMemset(m->d_chan_last, 0xff, C * 4));
    MFM_RUN_TRY(hipMalloc(&m->d_ctl, 2 * 4));
    MFM_RUN_TRY(hipMemset(m->d_ctl, 0, 2 * 4));
    MFM_RUN_TRY(hipMalloc(&m->d_totals, 4 * 8));
    MFM_RUN_TRY(hipMemset(m->d_totals, 0, 4 * 8));
    MFM_RUN_TRY(hipMalloc(&m->d_slots, (size_t)cap_decs * 2));
    MFM_RUN_TRY(hipMalloc(&m->d_decs, (size_t)cap_decs * 2));
    MFM_RUN_TRY(hipDeviceSynchronize());
    return MFM_OK;
}

void mfm_runmm_destroy(struct mfm_runmm **pm)
{
    if (!pm || !*pm) {
        return;
    }
    mfm_runmm *m = *pm;
    (void)hipSetDevice(m->cfg.device);
    (void)hipDeviceSynchronize();
    (void)hipFree(m->d_chan[0]);
    (void)hipFree(m->d_chan[1]);
    (void)hipFree(m->d_run_state);
    (void)hipFree(m->d_out_runs);
    (void)hipFree(m->d_slot_base);
    (void)hipFree(m->d_chan_last);
    (void)hipFree(m->d_ctl);
    (void)hipFree(m->d_totals);
    (void)hipFree(m->d_slots);
    (void)hipFree(m->d_decs);
    delete m;
    *pm = nullptr;
}

int mfm_runmm_process_device(struct mfm_runmm *m, const struct mfm_runrs_run *d_runs, const int16_t *d_payload, const uint64_t *d_totals,
                             void *stream)
{
    if (!m || !d_runs || !d_payload || !d_totals) {
        return MFM_E_INVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rb = mfm_run_call_begin(m, s);
    if (rb != MFM_OK) {
        return rb;
    }
    const uint32_t cur = m->cur;
    const RmCall A{ d_runs,        d_payload,      d_totals,      m->d_chan[cur], m->d_chan[cur ^ 1u], m->d_run_state, m->d_out_runs,
                    m->d_slot_base, m->d_chan_last, m->d_ctl,      m->d_totals,    m->d_slots,          m->d_decs,
                    m->cfg.nr_channels, m->cfg.max_runs, m->cfg.max_out_samples, (uint32_t)m->cap_decs, m->P };
    hipLaunchKernelGGL(rm_plan_kernel, dim3(1), dim3(MFM_RUN_SCAN_THREADS), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rm_walk_kernel, dim3((m->cfg.max_runs + RM_RUNS - 1u) / RM_RUNS), dim3(64), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rm_scan_kernel, dim3(1), dim3(MFM_RUN_SCAN_THREADS), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rm_compact_kernel, dim3(m->cfg.max_runs), dim3(64), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rm_state_kernel, dim3((m->cfg.nr_channels + 255u) / 256u), dim3(256), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    mfm_run_call_end(m, s);
    return MFM_OK;
}

int mfm_runmm_fetch(struct mfm_runmm *m, struct mfm_runmm_run *runs, size_t max_runs, size_t *nr_runs, int16_t *decisions,
                    size_t max_decisions, size_t *nr_decisions)
{
    if (!m || !nr_runs || !nr_decisions || (!runs && max_runs) || (!decisions && max_decisions)) {
        return MFM_E_INVAL;
    }
    *nr_runs = 0;
    *nr_decisions = 0;
    if (!m->have_call) {
        return MFM_OK;
    }
    MFM_RUN_TRY(hipSetDevice(m->cfg.device));
    MFM_RUN_TRY(hipStreamSynchronize(m->last_stream));
    uint64_t t[4];
    MFM_RUN_TRY(hipMemcpy(t, m->d_totals, sizeof(t), hipMemcpyDeviceToHost));
    if (t[MFM_RUN_T_OVERFLOW] || t[MFM_RUN_T_INPUT]) {
        return mfm_run_fail(MFM_E_STATE, rm_refusal(t[MFM_RUN_T_OVERFLOW], t[MFM_RUN_T_INPUT]));
    }
    *nr_runs = (size_t)t[RM_T_RUNS];
    *nr_decisions = (size_t)t[RM_T_DECS];
    if (t[RM_T_RUNS] > max_runs || t[RM_T_DECS] > max_decisions) {
        return MFM_E_NOMEM;
    }
    if (t[RM_T_RUNS]) {
        MFM_RUN_TRY(hipMemcpy(runs, m->d_out_runs, (size_t)t[RM_T_RUNS] * sizeof(mfm_runmm_run), hipMemcpyDeviceToHost));
    }
    if (t[RM_T_DECS]) {
        MFM_RUN_TRY(hipMemcpy(decisions, m->d_decs, (size_t)t[RM_T_DECS] * 2, hipMemcpyDeviceToHost));
    }
    return MFM_OK;
}

int mfm_runmm_device_view(struct mfm_runmm *m, const struct mfm_runmm_run **d_runs, const int16_t **d_decisions, const uint64_t **d_totals)
{
    if (!m) {
        return MFM_E_INVAL;
    }
    if (d_runs) {
        *d_runs = m->d_out_runs;
    }
    if (d_decisions) {
        *d_decisions = m->d_decs;
    }
    if (d_totals) {
        *d_totals = m->d_totals;
    }
    return MFM_OK;
}

int mfm_runmm_get_capacity(struct mfm_runmm *m, uint32_t *max_runs, uint64_t *max_decisions)
{
    if (!m) {
        return MFM_E_INVAL;
    }
    if (max_runs) {
        *max_runs = m->cfg.max_runs;
    }
    if (max_decisions) {
        *max_decisions = m->cap_decs;
    }
    return MFM_OK;
}

int mfm_runmm_fetch_state(struct mfm_runmm *m, struct mfm_runmm_state *state, size_t nr_channels)
{
    return mfm_run_fetch_state(m, state, nr_channels);
}

int mfm_hosttwin_runmm_state_check(uint32_t nr_channels, const struct mfm_runmm_state *state)
{
    return mfm_run_state_check(nr_channels, state, "Mueller-Muller", mfm_runmm_state_check);
}

int mfm_runmm_store_state(struct mfm_runmm *m, const struct mfm_runmm_state *state, size_t nr_channels)
{
    return mfm_run_store_state(m, state, nr_channels, mfm_hosttwin_runmm_state_check);
}

/* ---- the host twin: the same plan, the loop one decision at a time ---- */

int mfm_hosttwin_runmm_call(const struct mfm_runmm_config *cfg, struct mfm_runmm_state *state, const struct mfm_runrs_run *runs,
                            const int16_t *payload, const uint64_t *totals, struct mfm_runmm_run *out_runs, size_t max_out_runs,
                            size_t *nr_runs, int16_t *decisions, size_t max_out_decisions, size_t *nr_decisions, uint32_t *flags)
{
    if (!cfg || !state || !totals || !nr_runs || !nr_decisions || (!out_runs && max_out_runs) || (!decisions && max_out_decisions)) {
        return MFM_E_INVAL;
    }
    *nr_runs = 0;
    *nr_decisions = 0;
    if (flags) {
        *flags = 0;
    }
    mfm_runmm_params P{};
    uint64_t cap_decs = 0;
    const int rc = rm_geometry(*cfg, &P, &cap_decs);
    if (rc != MFM_OK) {
        return rc;
    }
    uint64_t n, over, err, ts = 0; /* the plan pass */
    if (!mfm_run_twin_plan(totals, cfg->nr_channels, cfg->max_runs, cfg->max_out_samples, state, runs, payload, false,
                           [&](uint32_t nr_out) { ts += mfm_runmm_slots(nr_out, P.s); }, &n, &over, &err)) {
        return MFM_E_INVAL;
    }
    if (!err && ts > cap_decs) {
        over = MFM_RUNMM_OVER_DECISIONS;
    }
    if (over || err) {
        return mfm_run_twin_refuse(over, err, flags, rm_refusal(over, err));
    }
    /* every run from the state the call started with (only a channel's first run reads it); the state its last run leaves */
    std::vector<mfm_runmm_run> recs(n);
    std::vector<mfm_runmm_state> left(n);
    std::vector<int16_t> out;
    for (uint64_t r = 0; r < n; r++) {
        const mfm_runrs_run &run = runs[r];
        mfm_runmm_state st = mfm_runmm_start(state[run.channel], run, P.spb);
        mfm_runmm_carry k{ st.w, st.m, st.last_sample, mfm_runmm_sign(st.last_sample) };
        const int16_t *x = payload + run.out_offset;
        mfm_runmm_run &o = recs[r];
        o.first_window = run.first_window;
        o.dec_offset = out.size();
        o.first_dec = st.decs;
        o.channel = run.channel;
        o.flags = run.flags & MFM_RUNRS_BEGINS;
        o.reserved = 0;
        uint32_t idx = st.next_offset, nd = 0;
        while (idx < run.nr_out) {
            out.push_back(x[idx]);
            nd++;
            idx += mfm_runmm_step(k, P, x[idx]);
        }
        o.nr_dec = nd;
        mfm_runmm_leave(st, k, idx, run.nr_out, nd);
        left[r] = st;
    }
    *nr_runs = (size_t)n;
    *nr_decisions = out.size();
    if (n > max_out_runs || out.size() > max_out_decisions) {
        return MFM_E_NOMEM; /* nothing written, the state included */
    }
    for (uint64_t r = 0; r < n; r++) {
        if (r + 1 == n || runs[r + 1].channel != runs[r].channel) {
            state[runs[r].channel] = left[r];
        }
    }
    if (n) {
        memcpy(out_runs, recs.data(), (size_t)n * sizeof(mfm_runmm_run));
    }
    if (!out.empty()) {
        memcpy(decisions, out.data(), out.size() * 2);
    }
    return MFM_OK;
}

} /* extern "C" */
