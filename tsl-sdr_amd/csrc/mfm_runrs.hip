/*
 * mfm_runrs.hip - the burst resampler: the runs the squelch gate left in its dense payload go through the rational resampler
 * (filter/polyphase_fir.c:162-233) on the device, one fresh resampler per stretch of consecutive windows of a channel.  See
 * include/multifm_hip.h for the boundary, mfm_runrs.h for the arithmetic, mfm_rs_plan.h for the phase length and the ratios
 * that are refused.
 *
 * The input is what mfm_gate_device_view returns; how many runs and samples a call carries is read on the device, so the
 * host never waits and every launch is sized from the capacities fixed at create.
 *
 *   rr_plan_kernel   one lane per run.  A run that is its channel's first of the call and whose first_window is the number
 *                    the channel expects continues the stretch (phase, pending samples, outputs so far from the channel's
 *                    state); every other run begins one.  nr_out in closed form (mfm_runrs_plan_run), the descriptor, the
 *                    run's count of workgroups for the FIR kernel; a channel's last run leaves its index for the state kernel.
 *   rr_scan_kernel   one block: exclusive scan of nr_out (out_offset) and of the workgroup counts over all runs (a thread
 *                    sums a stretch of runs, the waves scan by lane shifts, the 16 wave sums go through LDS), the totals and
 *                    the flags.  No atomics.
 *   rr_fir_kernel    the hot path.  A workgroup takes 1024 consecutive outputs of one run, which it finds from its index by
 *                    binary search in the scanned workgroup counts.  It stages the coefficient pairs and its input window -
 *                    the channel's pending samples, then the run's payload samples - into LDS: the window is laid out so
 *                    that every group of eight samples is 16 bytes in the payload too, and a group that lies wholly in the
 *                    run is one 16-byte load, the others (the pending samples, the run's ends) go one by one.  A thread
 *                    computes four outputs 256 apart as v_dot2_i32_i16 over sample pairs with wrapping int32; where
 *                    256 D is a multiple of I they share a phase and its pairs sit in registers (NP = 4 .. 32, as the NP
 *                    instances of mfm_resampler.hip), otherwise the pairs are read from LDS (NP = 0).
 *   rr_state_kernel  one block per channel: the state the channel's last run leaves (expected window, phase, outputs,
 *                    pending samples) goes into the OTHER of two state buffers; a channel without a run, and every channel
 *                    when the call raised a flag, copies its state over.  The buffers are used in turn, so the FIR kernel
 *                    and this one read the old state while the new one is written.
 *
 *   rr_dc_kernel     (mfm_runrs_dc.hip) only with the DC blocker on (mfm_runrs_set_dc_block), between the FIR and the state
 *                    kernel: one lane per run, in place on the output payload, one fresh blocker per stretch
 *                    (mfm_runrs_dc.h).  The full-row form (mfm_dc_block_kernel) is a dependent chain with one lane per
 *                    channel; here every run starts from a state
 *                    that is known before the call - zeros, or the channel's from the call before - so the runs of a call are
 *                    independent chains.  The blocker's state is kept in two buffers used in turn like the resampler's: a
 *                    channel's first run reads the old one, its last run writes the new one (they may be lanes of different
 *                    waves, so one buffer updated in place would be a race), and the state kernel copies over the channels
 *                    without a run and every channel of a refused call.
 *
 * The bodies of the scan and the FIR kernel are in mfm_runrs_kernels.h, with the form as a template parameter; this file holds
 * their PCM instances, mfm_run_bits.hip the bits form's (rrb_scan_kernel, rrb_fir_kernel), so neither form pays for the other.
 * The bits form (mfm_runrs_process_bits_device) is the same four kernels with the store replaced: the scan also scans the
 * runs' word counts (mfm_runrs_bit_words) into out_offset, and the FIR kernel ballots the predicate of the rounded output.
 * A thread's output u is tid + 256 u, so wave w holds outputs 256 u + 64 w .. + 63 of the workgroup: one ballot is two
 * finished words of the run's bit payload, which lane 0 stores.  Workgroup bases are multiples of 1024 outputs and every
 * run's bits start on a word, so no word is shared between workgroups or runs; lanes past the run's end contribute 0,
 * which is what zeroes the tail of its last word.
 *
 * The view entries (mfm_runrs_process_view_device, mfm_runrs_process_bits_view_device: a resampler sized to a local route of the
 * run router reads the gate's payload in place) queue rrv_plan_kernel (mfm_runrs_view.hip) in the place of rr_plan_kernel - the
 * same body, with a run's range checked against a bound of its own instead of the totals' elements - and everything else as it is.
 *
 * Nothing is floating point and nothing goes through an atomic.
 */
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/multifm_hip.h"

extern "C" __attribute__((visibility("hidden"))) void mfm_internal_set_error(const char *msg);
#include "mfm_numerics.h"
#include "mfm_rs_plan.h"
#include "mfm_runrs.h"
#include "mfm_runrs_dc.h"
#include "mfm_runrs_kernels.h"

/* the bits form's scan and FIR kernels (mfm_run_bits.hip), queued on s between the plan and the state kernel */
extern "C" __attribute__((visibility("hidden"))) int mfm_internal_runrs_bits_launch(const void *call, uint32_t np, uint32_t max_blocks,
                                                                                   uint32_t lds_bytes, hipStream_t s);

/* the DC blocker's kernel (mfm_runrs_dc.hip), queued on s between the FIR and the state kernel */
extern "C" __attribute__((visibility("hidden"))) int mfm_internal_runrs_dc_launch(const void *call, uint32_t cap_runs, hipStream_t s);

/* the view entries' plan kernel (mfm_runrs_view.hip), queued on s in the place of rr_plan_kernel */
extern "C" __attribute__((visibility("hidden"))) int mfm_internal_runrs_view_plan_launch(const void *call, const uint64_t *d_payload_elems,
                                                                                        uint32_t cap_runs, hipStream_t s);

namespace {

constexpr uint32_t RR_MAX_RATIO_TERM = 1u << 20;                     /* I and D at most: 1024 D + I stays far below 2^32 */
constexpr uint64_t RR_MAX_OUT = 1ull << 31;                          /* output elements per call at most */

/* everything create derives from the configuration and the taps, without a device */
struct RrGeom {
    uint32_t C = 0, W = 0, I = 0, D = 0, plen = 0, np = 0;
    uint32_t coef_bytes = 0, x_cap = 0, lds_bytes = 0;
    uint64_t cap_windows = 0, cap_runs = 0, cap_elems = 0, out_cap = 0, max_blocks = 0;
    RsPlan rs;
    char err[224] = "";
};

int rr_geometry(const mfm_runrs_config &cfg, const int16_t *coeffs, size_t nr_coeffs, bool with_caps, RrGeom &g)
{
    if (cfg.abi_version != MFM_ABI_VERSION || 0 == cfg.nr_channels || cfg.nr_channels > 65535u) {
        snprintf(g.err, sizeof(g.err), "abi_version or nr_channels (1 .. 65535) out of range");
        return MFM_E_INVAL;
    }
    if (cfg.flags != 0) {
        snprintf(g.err, sizeof(g.err), "flags must be 0: the burst resampler has no DC blocker and no sign-bit output");
        return MFM_E_INVAL;
    }
    if (0 == cfg.interpolate || 0 == cfg.decimate || cfg.interpolate > RR_MAX_RATIO_TERM || cfg.decimate > RR_MAX_RATIO_TERM) {
        snprintf(g.err, sizeof(g.err), "interpolate and decimate must be 1 .. %u", RR_MAX_RATIO_TERM);
        return MFM_E_INVAL;
    }
    if (0 == cfg.window_samples || cfg.window_samples > (1u << 20)) {
        snprintf(g.err, sizeof(g.err), "window_samples must be 1 .. 2^20, the window of a gate with elems_per_sample == 1 (PCM payloads only)");
        return MFM_E_INVAL;
    }
    if (!coeffs || !nr_coeffs) {
        snprintf(g.err, sizeof(g.err), "no taps");
        return MFM_E_INVAL;
    }
    /* [plen] and [walk]: mfm_rs_plan.h's rules, through its planner (the v_dot2 form, one sample per call: only these two
     * of its checks can fail) */
    mfm_resampler_config rc{};
    rc.abi_version = MFM_ABI_VERSION;
    rc.nr_channels = cfg.nr_channels;
    rc.interpolate = cfg.interpolate;
    rc.decimate = cfg.decimate;
    rc.max_in_samples = 1;
    rc.flags = MFM_RS_FORCE_DOT2;
    const int planned = rs_plan(rc, coeffs, nr_coeffs, g.rs);
    g.C = cfg.nr_channels;
    g.W = cfg.window_samples;
    g.I = cfg.interpolate;
    g.D = cfg.decimate;
    g.plen = g.rs.plen;
    /* LDS of a FIR workgroup: the coefficient image, then the input window of RR_OPB outputs.  The window begins up to 7
     * samples early (16-byte groups), its last output starts at most 1023 D / I + 1 samples in, reads plen samples and the
     * zero pairs that round NP up, and the whole is rounded up to eight: at most 1023 D / I + plen + 31 samples */
    const uint64_t coef = ((uint64_t)g.I * g.plen * 2u + 15u) & ~15ull;
    const uint64_t x_cap = (((uint64_t)RR_OPB * g.D) / g.I + g.plen + 40u) & ~7ull;
    if (g.plen && coef + x_cap * 2u > MFM_RUNRS_MAX_LDS_BYTES) {
        snprintf(g.err, sizeof(g.err),
                 "the coefficient image (%u phases of %u taps: %llu bytes) and the input window of a workgroup (%llu bytes) exceed "
                 "MFM_RUNRS_MAX_LDS_BYTES = %u bytes of LDS",
                 g.I, g.plen, (unsigned long long)coef, (unsigned long long)(x_cap * 2u), MFM_RUNRS_MAX_LDS_BYTES);
        return MFM_E_INVAL;
    }
    if (planned != MFM_OK) {
        snprintf(g.err, sizeof(g.err), "%s", g.rs.err[0] ? g.rs.err : "the resampler's planner refuses this ratio and these taps");
        return MFM_E_INVAL;
    }
    g.coef_bytes = (uint32_t)coef;
    g.x_cap = (uint32_t)x_cap;
    g.lds_bytes = (uint32_t)(coef + x_cap * 2u);
    const bool reg_coef = ((uint64_t)RR_NT * g.D) % g.I == 0 && g.plen / 2u <= RS_PAIRS_MAX;
    g.np = reg_coef ? ((g.plen / 2u + 3u) / 4u) * 4u : 0u;
    if (!with_caps) {
        return MFM_OK;
    }
    /* capacities: what one gate call can hand over */
    mfm_runrs_caps caps;
    if (!mfm_runrs_caps_of(g.C, g.W, cfg.max_windows, cfg.max_runs, cfg.max_in_samples, cfg.preroll_windows, caps)) {
        snprintf(g.err, sizeof(g.err), "max_windows or max_runs is 0 (the gate's default) and max_in_samples is 0: give the gate's max_in_samples");
        return MFM_E_INVAL;
    }
    g.cap_windows = caps.windows;
    g.cap_runs = caps.runs;
    g.cap_elems = g.cap_windows * g.W;
    /* a run of n samples that meets p <= plen pending ones produces at most (n + p) I / D + 1 outputs */
    g.out_cap = ((g.cap_elems + g.cap_runs * g.plen) * g.I) / g.D + g.cap_runs;
    g.max_blocks = g.out_cap / RR_OPB + g.cap_runs; /* a run of n outputs takes n / RR_OPB + 1 workgroups at most */
    if (g.cap_runs >= RR_MAX_OUT || g.cap_elems >= (1ull << 40) || g.out_cap >= RR_MAX_OUT || g.max_blocks >= RR_MAX_OUT) {
        snprintf(g.err, sizeof(g.err), "max_windows * window_samples * interpolate / decimate must stay below 2^31 output samples per call (%llu)",
                 (unsigned long long)g.out_cap);
        return MFM_E_INVAL;
    }
    return MFM_OK;
}

__global__ __launch_bounds__(256) void rr_plan_kernel(const RrCall A)
{
    rr_plan_body<false>(A, nullptr);
}

__global__ __launch_bounds__(RR_SCAN_THREADS) void rr_scan_kernel(const RrCall A)
{
    rr_scan_body<false>(A);
}

template <int NP>
__global__ __launch_bounds__(RR_NT) void rr_fir_kernel(const RrCall A)
{
    rr_fir_body<NP, false>(A);
}

__global__ __launch_bounds__(64) void rr_state_kernel(const RrCall A)
{
    __shared__ uint32_t s_last;
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        s_last = A.chan_last[c];
        A.chan_last[c] = RR_NONE; /* for the next call */
    }
    __syncthreads();
    const uint32_t last = s_last;
    const bool refused = A.totals[RR_T_OVERFLOW] != 0 || A.totals[RR_T_GATE] != 0;
    const mfm_runrs_state old = A.chan_old[c];
    const int16_t *po = A.pend_old + (size_t)c * A.pend_stride;
    int16_t *pn = A.pend_new + (size_t)c * A.pend_stride;
    if (last == RR_NONE || refused) { /* the state stays */
        if (tid == 0) {
            A.chan_new[c] = old;
            if (A.dc_old) { /* the DC blocker's state likewise (a channel with a run: its last run's lane wrote it, rr_dc_kernel) */
                A.dc_new[c] = A.dc_old[c];
            }
        }
        for (uint32_t i = tid; i < old.pending; i += blockDim.x) {
            pn[i] = po[i];
        }
        return;
    }
    const mfm_gate_run g = A.gruns[last];
    const RrPlan P = A.plan[last];
    const uint64_t nsamp = (uint64_t)g.nr_windows * A.W;
    const mfm_runrs_step st = mfm_runrs_plan_run(A.I, A.D, A.plen, P.p0, P.pending, nsamp);
    if (tid == 0) {
        mfm_runrs_state nw;
        nw.expected = g.first_window + g.nr_windows;
        nw.outs = A.runs[last].first_out + st.nr_out;
        nw.phase = st.phase;
        nw.pending = st.pending;
        A.chan_new[c] = nw;
    }
    const int16_t *run = A.gpayload + g.payload_offset;
    for (uint32_t i = tid; i < st.pending; i += blockDim.x) { /* stored as received: inversion is applied on use */
        pn[i] = mfm_runrs_sample(po, P.pending, run, nsamp, (int64_t)(st.pos_end + i), false);
    }
}

thread_local char g_rr_error[256] = "";

int rr_fail(int code, const char *msg)
{
    snprintf(g_rr_error, sizeof(g_rr_error), "%s", msg);
    mfm_internal_set_error(g_rr_error);
    return code;
}

} /* namespace */

#define RR_TRY(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t err_ = (expr);                                                                            \
        if (err_ != hipSuccess) {                                                                            \
            snprintf(g_rr_error, sizeof(g_rr_error), "%s failed: %s", #expr, hipGetErrorString(err_));       \
            mfm_internal_set_error(g_rr_error);                                                              \
            return err_ == hipErrorOutOfMemory ? MFM_E_NOMEM : MFM_E_DEVICE;                                 \
        }                                                                                                    \
    } while (0)

struct mfm_runrs {
    mfm_runrs_config cfg{};
    RrGeom g;
    uint32_t pend_stride = 0;
    int16_t *d_phase = nullptr;
    mfm_runrs_state *d_chan[2] = { nullptr, nullptr }; /* used in turn: a call reads [cur] and writes [cur ^ 1] */
    int16_t *d_pend[2] = { nullptr, nullptr };
    mfm_runrs_dc_state *d_dc[2] = { nullptr, nullptr }; /* the DC blocker's, in turn with the two above; allocated by set_dc_block */
    uint32_t dc_on = 0;
    int32_t dc_p = 0;
    uint32_t cur = 0;
    RrPlan *d_plan = nullptr;
    uint32_t *d_nblk = nullptr, *d_blk_base = nullptr, *d_bad = nullptr, *d_chan_last = nullptr, *d_ctl = nullptr;
    uint64_t *d_totals = nullptr;
    mfm_runrs_run *d_runs = nullptr;
    int16_t *d_out = nullptr;
    uint32_t *d_bits = nullptr; /* the bits form's payload, bits_cap words */
    uint64_t bits_cap = 0;
    uint32_t last_polarity = 0; /* of the last call: 0 = the PCM form */
    hipStream_t last_stream = nullptr;
    bool have_call = false;
};

namespace {

void rr_launch_fir(const RrGeom &g, const RrCall &A, hipStream_t s)
{
    const dim3 grid((uint32_t)g.max_blocks);
    switch (g.np / 4u) {
    case 1: hipLaunchKernelGGL((rr_fir_kernel<4>), grid, dim3(RR_NT), g.lds_bytes, s, A); break;
    case 2: hipLaunchKernelGGL((rr_fir_kernel<8>), grid, dim3(RR_NT), g.lds_bytes, s, A); break;
    case 3: hipLaunchKernelGGL((rr_fir_kernel<12>), grid, dim3(RR_NT), g.lds_bytes, s, A); break;
    case 4: hipLaunchKernelGGL((rr_fir_kernel<16>), grid, dim3(RR_NT), g.lds_bytes, s, A); break;
    case 5: hipLaunchKernelGGL((rr_fir_kernel<20>), grid, dim3(RR_NT), g.lds_bytes, s, A); break;
    case 6: hipLaunchKernelGGL((rr_fir_kernel<24>), grid, dim3(RR_NT), g.lds_bytes, s, A); break;
    case 7: hipLaunchKernelGGL((rr_fir_kernel<28>), grid, dim3(RR_NT), g.lds_bytes, s, A); break;
    case 8: hipLaunchKernelGGL((rr_fir_kernel<32>), grid, dim3(RR_NT), g.lds_bytes, s, A); break;
    default: hipLaunchKernelGGL((rr_fir_kernel<0>), grid, dim3(RR_NT), g.lds_bytes, s, A); break;
    }
}

/* one call in either form: polarity 0 is the PCM form.  view: the view entries, whose plan kernel (mfm_runrs_view.hip) checks a
 * run's payload range against *d_payload_elems; everything behind it is queued as without */
int rr_process(mfm_runrs *rr, const mfm_gate_run *d_runs, const int16_t *d_payload, const uint64_t *d_totals, uint32_t polarity, void *stream,
               bool view = false, const uint64_t *d_payload_elems = nullptr)
{
    if (!rr || !d_runs || !d_payload || !d_totals || (view && !d_payload_elems)) {
        return MFM_E_INVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    RR_TRY(hipSetDevice(rr->cfg.device));
    if (rr->have_call && rr->last_stream != s) {
        RR_TRY(hipStreamSynchronize(rr->last_stream)); /* state lives on the device; keep calls ordered */
    }
    const RrGeom &g = rr->g;
    const uint32_t cur = rr->cur;
    const bool bits = polarity != 0;
    const RrCall A{ d_runs,      d_payload,       d_totals,  rr->d_chan[cur], rr->d_chan[cur ^ 1u], rr->d_pend[cur], rr->d_pend[cur ^ 1u],
                    rr->d_phase, rr->d_runs,      rr->d_plan, rr->d_nblk,     rr->d_blk_base,       rr->d_bad,       rr->d_chan_last,
                    rr->d_ctl,   rr->d_totals,    rr->d_out, g.cap_runs,      g.cap_elems,          g.out_cap,       g.C,
                    g.W,         g.I,             g.D,       g.plen,          rr->pend_stride,      rr->cfg.invert,  g.coef_bytes,
                    rr->d_bits,  polarity,        rr->dc_on ? rr->d_dc[cur] : nullptr,      rr->dc_on ? rr->d_dc[cur ^ 1u] : nullptr,
                    rr->dc_p };
    if (g.cap_runs && view) {
        if (mfm_internal_runrs_view_plan_launch(&A, d_payload_elems, (uint32_t)g.cap_runs, s) != MFM_OK) {
            RR_TRY(hipGetLastError());
            return MFM_E_DEVICE;
        }
    } else if (g.cap_runs) {
        hipLaunchKernelGGL(rr_plan_kernel, dim3((uint32_t)((g.cap_runs + 255u) / 256u)), dim3(256), 0, s, A);
        RR_TRY(hipGetLastError());
    }
    if (bits) {
        if (mfm_internal_runrs_bits_launch(&A, g.np, (uint32_t)g.max_blocks, g.lds_bytes, s) != MFM_OK) {
            RR_TRY(hipGetLastError());
            return MFM_E_DEVICE;
        }
    } else {
        hipLaunchKernelGGL(rr_scan_kernel, dim3(1), dim3(RR_SCAN_THREADS), 0, s, A);
        RR_TRY(hipGetLastError());
        if (g.max_blocks) {
            rr_launch_fir(g, A, s);
            RR_TRY(hipGetLastError());
        }
        if (rr->dc_on && g.cap_runs) { /* run count and flags are read on the device: sized from the capacity */
            if (mfm_internal_runrs_dc_launch(&A, (uint32_t)g.cap_runs, s) != MFM_OK) {
                RR_TRY(hipGetLastError());
                return MFM_E_DEVICE;
            }
        }
    }
    hipLaunchKernelGGL(rr_state_kernel, dim3(g.C), dim3(64), 0, s, A);
    RR_TRY(hipGetLastError());
    rr->cur ^= 1u;
    rr->last_stream = s;
    rr->have_call = true;
    rr->last_polarity = polarity;
    return MFM_OK;
}

/* the message of a refused call, from its totals (NULL: the call was not refused) */
const char *rr_refusal(const uint64_t *t)
{
    if (t[RR_T_GATE] & MFM_RUNRS_GATE_OUT_OF_STEP) {
        return "the gate's call was out of step with its level stage";
    }
    if (t[RR_T_GATE]) {
        return "the run list is not a gate's: a run names a channel or a payload range that does not exist";
    }
    if (t[RR_T_OVERFLOW] & MFM_RUNRS_OVER_GATE) {
        return "the gate's call overflowed its max_open_windows";
    }
    if (t[RR_T_OVERFLOW]) {
        return "the gate's call exceeds max_windows or max_runs";
    }
    return nullptr;
}

constexpr const char *RR_BAD_POLE = "the DC blocker's pole must be a number whose (1 - pole) * 16384 fits the int16 it is cut to (filter/dc_blocker.h:56)";
constexpr const char *RR_LAST_WAS_BITS = "the last call was mfm_runrs_process_bits_device: its result is read with mfm_runrs_fetch_bits or mfm_runrs_bits_view";
constexpr const char *RR_LAST_WAS_PCM = "the last call was not mfm_runrs_process_bits_device: its result is read with mfm_runrs_fetch or mfm_runrs_device_view";

} /* namespace */

extern "C" {

int mfm_runrs_create(struct mfm_runrs **prr, const struct mfm_runrs_config *cfg, const int16_t *coeffs, size_t nr_coeffs)
{
    if (!prr || !cfg) {
        return MFM_E_INVAL;
    }
    *prr = nullptr;
    mfm_runrs *rr = new (std::nothrow) mfm_runrs();
    if (!rr) {
        return MFM_E_NOMEM;
    }
    if (rr_geometry(*cfg, coeffs, nr_coeffs, true, rr->g) != MFM_OK) {
        const int rc = rr_fail(MFM_E_INVAL, rr->g.err);
        delete rr;
        return rc;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) {
        delete rr;
        return MFM_E_DEVICE; /* no CPU path */
    }
    rr->cfg = *cfg;
    const RrGeom &g = rr->g;
    RsTables tab;
    rs_build_tables(g.rs, coeffs, tab);
    std::vector<mfm_runrs_state> fresh(g.C);
    for (auto &st : fresh) {
        st = mfm_runrs_state{ MFM_RUNRS_NO_WINDOW, 0, 0, 0 };
    }
    rr->pend_stride = (g.plen + 7u) & ~7u;
    const size_t nruns = (size_t)(g.cap_runs ? g.cap_runs : 1), nout = (size_t)(g.out_cap ? g.out_cap : 1);
    *prr = rr; /* from here on the caller's destroy frees what was allocated */
    RR_TRY(hipSetDevice(cfg->device));
    RR_TRY(hipMalloc(&rr->d_phase, tab.phase.size() * 2));
    RR_TRY(hipMemcpy(rr->d_phase, tab.phase.data(), tab.phase.size() * 2, hipMemcpyHostToDevice));
    for (int i = 0; i < 2; i++) {
        RR_TRY(hipMalloc(&rr->d_chan[i], (size_t)g.C * sizeof(mfm_runrs_state)));
        RR_TRY(hipMemcpy(rr->d_chan[i], fresh.data(), (size_t)g.C * sizeof(mfm_runrs_state), hipMemcpyHostToDevice));
        RR_TRY(hipMalloc(&rr->d_pend[i], (size_t)g.C * rr->pend_stride * 2));
        RR_TRY(hipMemset(rr->d_pend[i], 0, (size_t)g.C * rr->pend_stride * 2));
    }
    RR_TRY(hipMalloc(&rr->d_plan, nruns * sizeof(RrPlan)));
    RR_TRY(hipMalloc(&rr->d_nblk, nruns * 4));
    RR_TRY(hipMalloc(&rr->d_blk_base, (nruns + 1) * 4));
    RR_TRY(hipMalloc(&rr->d_bad, nruns * 4));
    RR_TRY(hipMalloc(&rr->d_chan_last, (size_t)g.C * 4));
    RR_TRY(hipMemset(rr->d_chan_last, 0xff, (size_t)g.C * 4));
    RR_TRY(hipMalloc(&rr->d_ctl, 2 * 4));
    RR_TRY(hipMemset(rr->d_ctl, 0, 2 * 4));
    RR_TRY(hipMalloc(&rr->d_totals, 4 * 8));
    RR_TRY(hipMemset(rr->d_totals, 0, 4 * 8));
    RR_TRY(hipMalloc(&rr->d_runs, nruns * sizeof(mfm_runrs_run)));
    RR_TRY(hipMalloc(&rr->d_out, nout * 2));
    rr->bits_cap = g.out_cap / 32u + g.cap_runs; /* a run of n outputs owns n / 32 words and at most one more */
    RR_TRY(hipMalloc(&rr->d_bits, (size_t)(rr->bits_cap ? rr->bits_cap : 1) * 4));
    RR_TRY(hipDeviceSynchronize());
    return MFM_OK;
}

void mfm_runrs_destroy(struct mfm_runrs **prr)
{
    if (!prr || !*prr) {
        return;
    }
    mfm_runrs *rr = *prr;
    (void)hipSetDevice(rr->cfg.device);
    (void)hipDeviceSynchronize();
    (void)hipFree(rr->d_phase);
    for (int i = 0; i < 2; i++) {
        (void)hipFree(rr->d_chan[i]);
        (void)hipFree(rr->d_pend[i]);
        (void)hipFree(rr->d_dc[i]);
    }
    (void)hipFree(rr->d_plan);
    (void)hipFree(rr->d_nblk);
    (void)hipFree(rr->d_blk_base);
    (void)hipFree(rr->d_bad);
    (void)hipFree(rr->d_chan_last);
    (void)hipFree(rr->d_ctl);
    (void)hipFree(rr->d_totals);
    (void)hipFree(rr->d_runs);
    (void)hipFree(rr->d_out);
    (void)hipFree(rr->d_bits);
    delete rr;
    *prr = nullptr;
}

int mfm_runrs_process_device(struct mfm_runrs *rr, const struct mfm_gate_run *d_runs, const int16_t *d_payload, const uint64_t *d_totals,
                             void *stream)
{
    return rr_process(rr, d_runs, d_payload, d_totals, 0, stream);
}

int mfm_runrs_process_bits_device(struct mfm_runrs *rr, const struct mfm_gate_run *d_runs, const int16_t *d_payload,
                                  const uint64_t *d_totals, uint32_t polarity, void *stream)
{
    if (polarity != MFM_BITS_NEG && polarity != MFM_BITS_POS) {
        return rr_fail(MFM_E_INVAL, "polarity must be MFM_BITS_NEG or MFM_BITS_POS");
    }
    if (rr && rr->dc_on) {
        return rr_fail(MFM_E_INVAL, "the sign-bit output is not available with the DC blocker: it filters the PCM the predicate would be "
                                    "taken from (mfm_runrs_process_device, or mfm_runrs_set_dc_block off)");
    }
    return rr_process(rr, d_runs, d_payload, d_totals, polarity, stream);
}

int mfm_runrs_process_view_device(struct mfm_runrs *rr, const struct mfm_gate_run *d_runs, const int16_t *d_payload, const uint64_t *d_totals,
                                  const uint64_t *d_payload_elems, void *stream)
{
    return rr_process(rr, d_runs, d_payload, d_totals, 0, stream, true, d_payload_elems);
}

int mfm_runrs_process_bits_view_device(struct mfm_runrs *rr, const struct mfm_gate_run *d_runs, const int16_t *d_payload,
                                       const uint64_t *d_totals, const uint64_t *d_payload_elems, uint32_t polarity, void *stream)
{
    if (polarity != MFM_BITS_NEG && polarity != MFM_BITS_POS) {
        return rr_fail(MFM_E_INVAL, "polarity must be MFM_BITS_NEG or MFM_BITS_POS");
    }
    if (rr && rr->dc_on) {
        return rr_fail(MFM_E_INVAL, "the sign-bit output is not available with the DC blocker: it filters the PCM the predicate would be "
                                    "taken from (mfm_runrs_process_view_device, or mfm_runrs_set_dc_block off)");
    }
    return rr_process(rr, d_runs, d_payload, d_totals, polarity, stream, true, d_payload_elems);
}

int mfm_runrs_set_dc_block(struct mfm_runrs *rr, uint32_t on, double pole)
{
    if (!rr) {
        return MFM_E_INVAL;
    }
    if (rr->have_call) {
        return rr_fail(MFM_E_STATE, "mfm_runrs_set_dc_block is valid only before the first process call");
    }
    if (!on) {
        rr->dc_on = 0;
        rr->dc_p = 0;
        return MFM_OK;
    }
    int32_t p = 0;
    if (!mfm_runrs_dc_pole(pole, &p)) {
        return rr_fail(MFM_E_INVAL, RR_BAD_POLE);
    }
    RR_TRY(hipSetDevice(rr->cfg.device));
    for (int i = 0; i < 2; i++) {
        if (!rr->d_dc[i]) {
            RR_TRY(hipMalloc(&rr->d_dc[i], (size_t)rr->g.C * sizeof(mfm_runrs_dc_state)));
        }
        RR_TRY(hipMemset(rr->d_dc[i], 0, (size_t)rr->g.C * sizeof(mfm_runrs_dc_state)));
    }
    RR_TRY(hipDeviceSynchronize());
    rr->dc_on = 1;
    rr->dc_p = p;
    return MFM_OK;
}

int mfm_runrs_get_dc_block(struct mfm_runrs *rr, uint32_t *on, int32_t *dc_p)
{
    if (!rr) {
        return MFM_E_INVAL;
    }
    if (on) {
        *on = rr->dc_on;
    }
    if (dc_p) {
        *dc_p = rr->dc_p;
    }
    return MFM_OK;
}

int mfm_runrs_fetch(struct mfm_runrs *rr, struct mfm_runrs_run *runs, size_t max_runs, size_t *nr_runs, int16_t *payload, size_t max_elems,
                    size_t *nr_elems)
{
    if (!rr || !nr_runs || !nr_elems || (!runs && max_runs) || (!payload && max_elems)) {
        return MFM_E_INVAL;
    }
    *nr_runs = 0;
    *nr_elems = 0;
    if (!rr->have_call) {
        return MFM_OK;
    }
    if (rr->last_polarity) {
        return rr_fail(MFM_E_STATE, RR_LAST_WAS_BITS);
    }
    RR_TRY(hipSetDevice(rr->cfg.device));
    RR_TRY(hipStreamSynchronize(rr->last_stream));
    uint64_t t[4];
    RR_TRY(hipMemcpy(t, rr->d_totals, sizeof(t), hipMemcpyDeviceToHost));
    *nr_runs = (size_t)t[RR_T_RUNS];
    *nr_elems = (size_t)t[RR_T_ELEMS];
    if (const char *why = rr_refusal(t)) {
        return rr_fail(MFM_E_STATE, why);
    }
    if (t[RR_T_RUNS] > max_runs || t[RR_T_ELEMS] > max_elems) {
        return MFM_E_NOMEM;
    }
    if (t[RR_T_RUNS]) {
        RR_TRY(hipMemcpy(runs, rr->d_runs, (size_t)t[RR_T_RUNS] * sizeof(mfm_runrs_run), hipMemcpyDeviceToHost));
    }
    if (t[RR_T_ELEMS]) {
        RR_TRY(hipMemcpy(payload, rr->d_out, (size_t)t[RR_T_ELEMS] * 2, hipMemcpyDeviceToHost));
    }
    return MFM_OK;
}

int mfm_runrs_device_view(struct mfm_runrs *rr, const struct mfm_runrs_run **d_runs, const int16_t **d_payload, const uint64_t **d_totals)
{
    if (!rr) {
        return MFM_E_INVAL;
    }
    if (rr->have_call && rr->last_polarity) {
        return rr_fail(MFM_E_STATE, RR_LAST_WAS_BITS);
    }
    if (d_runs) {
        *d_runs = rr->d_runs;
    }
    if (d_payload) {
        *d_payload = rr->d_out;
    }
    if (d_totals) {
        *d_totals = rr->d_totals;
    }
    return MFM_OK;
}

int mfm_runrs_fetch_bits(struct mfm_runrs *rr, struct mfm_runrs_run *runs, size_t max_runs, size_t *nr_runs, uint32_t *bits, size_t max_words,
                         size_t *nr_words)
{
    if (!rr || !nr_runs || !nr_words || (!runs && max_runs) || (!bits && max_words)) {
        return MFM_E_INVAL;
    }
    *nr_runs = 0;
    *nr_words = 0;
    if (!rr->have_call) {
        return MFM_OK;
    }
    if (!rr->last_polarity) {
        return rr_fail(MFM_E_STATE, RR_LAST_WAS_PCM);
    }
    RR_TRY(hipSetDevice(rr->cfg.device));
    RR_TRY(hipStreamSynchronize(rr->last_stream));
    uint64_t t[4];
    RR_TRY(hipMemcpy(t, rr->d_totals, sizeof(t), hipMemcpyDeviceToHost));
    *nr_runs = (size_t)t[RR_T_RUNS];
    *nr_words = (size_t)t[RR_T_ELEMS];
    if (const char *why = rr_refusal(t)) {
        return rr_fail(MFM_E_STATE, why);
    }
    if (t[RR_T_RUNS] > max_runs || t[RR_T_ELEMS] > max_words) {
        return MFM_E_NOMEM;
    }
    if (t[RR_T_RUNS]) {
        RR_TRY(hipMemcpy(runs, rr->d_runs, (size_t)t[RR_T_RUNS] * sizeof(mfm_runrs_run), hipMemcpyDeviceToHost));
    }
    if (t[RR_T_ELEMS]) {
        RR_TRY(hipMemcpy(bits, rr->d_bits, (size_t)t[RR_T_ELEMS] * 4, hipMemcpyDeviceToHost));
    }
    return MFM_OK;
}

int mfm_runrs_bits_view(struct mfm_runrs *rr, struct mfm_runrs_bits_view *view)
{
    if (!rr || !view) {
        return MFM_E_INVAL;
    }
    if (!rr->have_call || !rr->last_polarity) {
        return rr_fail(MFM_E_STATE, RR_LAST_WAS_PCM);
    }
    view->d_runs = rr->d_runs;
    view->d_bits = rr->d_bits;
    view->d_totals = rr->d_totals;
    view->polarity = rr->last_polarity;
    view->reserved = 0;
    return MFM_OK;
}

int mfm_runrs_get_bits_capacity(struct mfm_runrs *rr, uint32_t *max_runs, uint64_t *max_words)
{
    if (!rr) {
        return MFM_E_INVAL;
    }
    if (max_runs) {
        *max_runs = (uint32_t)rr->g.cap_runs;
    }
    if (max_words) {
        *max_words = rr->bits_cap;
    }
    return MFM_OK;
}

int mfm_runrs_get_capacity(struct mfm_runrs *rr, uint32_t *max_runs, uint64_t *max_out_elems)
{
    if (!rr) {
        return MFM_E_INVAL;
    }
    if (max_runs) {
        *max_runs = (uint32_t)rr->g.cap_runs;
    }
    if (max_out_elems) {
        *max_out_elems = rr->g.out_cap;
    }
    return MFM_OK;
}

int mfm_hosttwin_runrs_state_check(uint32_t nr_channels, uint32_t interpolate, uint32_t plen, const struct mfm_runrs_state *state,
                                   const struct mfm_runrs_dc_state *dc)
{
    if (!state || !nr_channels) {
        return MFM_E_INVAL;
    }
    for (uint32_t c = 0; c < nr_channels; c++) {
        const char *why = mfm_runrs_state_check(state[c], interpolate, plen);
        if (!why && dc) {
            why = mfm_runrs_dc_state_check(dc[c]);
        }
        if (why) {
            char msg[224];
            snprintf(msg, sizeof(msg), "burst resampler state, channel %u: %s", c, why);
            return rr_fail(MFM_E_INVAL, msg);
        }
    }
    return MFM_OK;
}

int mfm_runrs_fetch_state(struct mfm_runrs *rr, struct mfm_runrs_state *state, int16_t *pending, struct mfm_runrs_dc_state *dc,
                          size_t nr_channels)
{
    if (!rr || !state || nr_channels != rr->g.C) {
        return MFM_E_INVAL;
    }
    if (dc && !rr->dc_on) {
        return rr_fail(MFM_E_STATE, "the DC blocker is off: it has no state (mfm_runrs_set_dc_block)");
    }
    RR_TRY(hipSetDevice(rr->cfg.device));
    if (rr->have_call) {
        RR_TRY(hipStreamSynchronize(rr->last_stream));
    }
    const uint32_t cur = rr->cur;
    RR_TRY(hipMemcpy(state, rr->d_chan[cur], nr_channels * sizeof(mfm_runrs_state), hipMemcpyDeviceToHost));
    if (pending && rr->g.plen) {
        RR_TRY(hipMemcpy2D(pending, (size_t)rr->g.plen * 2, rr->d_pend[cur], (size_t)rr->pend_stride * 2, (size_t)rr->g.plen * 2, nr_channels,
                           hipMemcpyDeviceToHost));
    }
    if (dc) {
        RR_TRY(hipMemcpy(dc, rr->d_dc[cur], nr_channels * sizeof(mfm_runrs_dc_state), hipMemcpyDeviceToHost));
    }
    return MFM_OK;
}

int mfm_runrs_store_state(struct mfm_runrs *rr, const struct mfm_runrs_state *state, const int16_t *pending,
                          const struct mfm_runrs_dc_state *dc, size_t nr_channels)
{
    if (!rr || !state || !pending || nr_channels != rr->g.C) {
        return MFM_E_INVAL;
    }
    if ((dc != nullptr) != (rr->dc_on != 0)) {
        return rr_fail(MFM_E_INVAL, rr->dc_on ? "the DC blocker is on: its state is required" : "the DC blocker is off: its state must be NULL");
    }
    const int ok = mfm_hosttwin_runrs_state_check(rr->g.C, rr->g.I, rr->g.plen, state, dc);
    if (ok != MFM_OK) {
        return ok;
    }
    RR_TRY(hipSetDevice(rr->cfg.device));
    if (rr->have_call) {
        RR_TRY(hipStreamSynchronize(rr->last_stream));
    }
    const uint32_t cur = rr->cur;
    RR_TRY(hipMemcpy(rr->d_chan[cur], state, nr_channels * sizeof(mfm_runrs_state), hipMemcpyHostToDevice));
    if (rr->g.plen) {
        RR_TRY(hipMemcpy2D(rr->d_pend[cur], (size_t)rr->pend_stride * 2, pending, (size_t)rr->g.plen * 2, (size_t)rr->g.plen * 2, nr_channels,
                           hipMemcpyHostToDevice));
    }
    if (dc) {
        RR_TRY(hipMemcpy(rr->d_dc[cur], dc, nr_channels * sizeof(mfm_runrs_dc_state), hipMemcpyHostToDevice));
    }
    return MFM_OK;
}

int mfm_hosttwin_runrs_plan(uint32_t interpolate, uint32_t decimate, uint32_t plen, const uint32_t *phase, const uint32_t *pending,
                            const uint64_t *nr_samples, size_t n, uint64_t *nr_out, uint32_t *phase_out, uint32_t *pending_out)
{
    if (!interpolate || !decimate || !plen || interpolate > RR_MAX_RATIO_TERM || decimate > RR_MAX_RATIO_TERM ||
        (decimate + interpolate - 1) / interpolate > plen || (n && (!phase || !pending || !nr_samples || !nr_out || !phase_out || !pending_out))) {
        return MFM_E_INVAL;
    }
    for (size_t i = 0; i < n; i++) {
        if (phase[i] >= interpolate || pending[i] > plen || nr_samples[i] >= (1ull << 40)) {
            return MFM_E_INVAL;
        }
    }
    for (size_t i = 0; i < n; i++) {
        const mfm_runrs_step st = mfm_runrs_plan_run(interpolate, decimate, plen, phase[i], pending[i], nr_samples[i]);
        nr_out[i] = st.nr_out;
        phase_out[i] = st.phase;
        pending_out[i] = st.pending;
    }
    return MFM_OK;
}

} /* extern "C" */

namespace {

/* the host twin of one call in either form: polarity 0 writes int16 into `payload`, otherwise predicate words into `bits` and
 * max_elems / *nr_elems count words */
int rr_twin_call(uint32_t nr_channels, uint32_t window_samples, uint32_t interpolate, uint32_t decimate, uint32_t invert, const int16_t *coeffs,
                 size_t nr_coeffs, struct mfm_runrs_state *state, int16_t *pending, const struct mfm_gate_run *gate_runs, size_t nr_gate_runs,
                 const int16_t *gate_payload, size_t nr_gate_elems, struct mfm_runrs_run *runs, size_t max_runs, size_t *nr_runs,
                 int16_t *payload, uint32_t *bits, uint32_t polarity, size_t max_elems, size_t *nr_elems)
{
    if (!state || !pending || !nr_runs || !nr_elems || (!gate_runs && nr_gate_runs) || (!gate_payload && nr_gate_elems) || (!runs && max_runs) ||
        (!payload && !bits && max_elems)) {
        return MFM_E_INVAL;
    }
    mfm_runrs_config cfg{};
    cfg.abi_version = MFM_ABI_VERSION;
    cfg.nr_channels = nr_channels;
    cfg.interpolate = interpolate;
    cfg.decimate = decimate;
    cfg.window_samples = window_samples;
    RrGeom g;
    if (rr_geometry(cfg, coeffs, nr_coeffs, false, g) != MFM_OK) {
        return rr_fail(MFM_E_INVAL, g.err);
    }
    RsTables tab;
    rs_build_tables(g.rs, coeffs, tab);
    const uint32_t I = g.I, D = g.D, plen = g.plen, W = g.W;
    /* the plan pass and the scan */
    std::vector<mfm_runrs_start> start(nr_gate_runs);
    std::vector<mfm_runrs_step> step(nr_gate_runs);
    uint64_t total = 0;
    for (size_t r = 0; r < nr_gate_runs; r++) {
        const mfm_gate_run &gr = gate_runs[r];
        const uint64_t nsamp = (uint64_t)gr.nr_windows * W;
        if (gr.channel >= nr_channels || gr.payload_offset > nr_gate_elems || nsamp > nr_gate_elems - gr.payload_offset) {
            return rr_fail(MFM_E_INVAL, "the run list is not a gate's: a run names a channel or a payload range that does not exist");
        }
        const bool first = r == 0 || gate_runs[r - 1].channel != gr.channel;
        start[r] = mfm_runrs_start_of(state[gr.channel], first, gr.first_window);
        step[r] = mfm_runrs_plan_run(I, D, plen, start[r].phase, start[r].pending, nsamp);
        total += polarity ? mfm_runrs_bit_words((uint32_t)step[r].nr_out) : step[r].nr_out;
    }
    *nr_runs = nr_gate_runs;
    *nr_elems = (size_t)total;
    if (nr_gate_runs > max_runs || total > max_elems) {
        return MFM_E_NOMEM; /* nothing written, the state included: the caller may call again */
    }
    /* the outputs, then the state each channel's last run leaves (which reads the old pending samples, as the outputs do) */
    uint64_t at = 0;
    for (size_t r = 0; r < nr_gate_runs; r++) {
        const mfm_gate_run &gr = gate_runs[r];
        const uint64_t nsamp = (uint64_t)gr.nr_windows * W;
        const int16_t *run = gate_payload + gr.payload_offset;
        const int16_t *pend = pending + (size_t)gr.channel * plen;
        mfm_runrs_run &o = runs[r];
        o.first_window = gr.first_window;
        o.out_offset = at;
        o.first_out = start[r].first_out;
        o.channel = gr.channel;
        o.nr_out = (uint32_t)step[r].nr_out;
        o.flags = start[r].begins ? MFM_RUNRS_BEGINS : 0u;
        o.reserved = 0;
        for (uint64_t j = 0; j < step[r].nr_out; j++) {
            const uint64_t t = start[r].phase + j * D, pos = t / I, ph = t - pos * I;
            uint32_t acc = 0; /* filter/utils.c:94-103, int32 wrap-around */
            for (uint32_t k = 0; k < plen; k++) {
                const int32_t x = mfm_runrs_sample(pend, start[r].pending, run, nsamp, (int64_t)(pos + k), invert != 0);
                acc += (uint32_t)(x * (int32_t)tab.phase[(size_t)ph * plen + k]);
            }
            const int16_t y = (int16_t)mfm_r14_wide((int32_t)acc); /* utils.c:112 */
            if (!polarity) {
                payload[at + j] = y;
            } else {
                if (j % 32u == 0) {
                    bits[at + j / 32u] = 0; /* the tail of the run's last word stays zero */
                }
                bits[at + j / 32u] |= (mfm_runrs_bit(y, polarity) ? 1u : 0u) << (j % 32u);
            }
        }
        at += polarity ? mfm_runrs_bit_words((uint32_t)step[r].nr_out) : step[r].nr_out;
    }
    std::vector<int16_t> keep(plen);
    for (size_t r = 0; r < nr_gate_runs; r++) {
        const mfm_gate_run &gr = gate_runs[r];
        if (r + 1 != nr_gate_runs && gate_runs[r + 1].channel == gr.channel) {
            continue;
        }
        const uint64_t nsamp = (uint64_t)gr.nr_windows * W;
        int16_t *pend = pending + (size_t)gr.channel * plen;
        for (uint32_t i = 0; i < step[r].pending; i++) {
            keep[i] = mfm_runrs_sample(pend, start[r].pending, gate_payload + gr.payload_offset, nsamp, (int64_t)(step[r].pos_end + i), false);
        }
        memcpy(pend, keep.data(), (size_t)step[r].pending * 2);
        mfm_runrs_state &st = state[gr.channel];
        st.expected = gr.first_window + gr.nr_windows;
        st.outs = start[r].first_out + step[r].nr_out;
        st.phase = step[r].phase;
        st.pending = step[r].pending;
    }
    return MFM_OK;
}

} /* namespace */

extern "C" {

int mfm_hosttwin_runrs_call(uint32_t nr_channels, uint32_t window_samples, uint32_t interpolate, uint32_t decimate, uint32_t invert,
                            const int16_t *coeffs, size_t nr_coeffs, struct mfm_runrs_state *state, int16_t *pending,
                            const struct mfm_gate_run *gate_runs, size_t nr_gate_runs, const int16_t *gate_payload, size_t nr_gate_elems,
                            struct mfm_runrs_run *runs, size_t max_runs, size_t *nr_runs, int16_t *payload, size_t max_elems,
                            size_t *nr_elems)
{
    return rr_twin_call(nr_channels, window_samples, interpolate, decimate, invert, coeffs, nr_coeffs, state, pending, gate_runs, nr_gate_runs,
                        gate_payload, nr_gate_elems, runs, max_runs, nr_runs, payload, nullptr, 0, max_elems, nr_elems);
}

int mfm_hosttwin_runrs_call_bits(uint32_t nr_channels, uint32_t window_samples, uint32_t interpolate, uint32_t decimate, uint32_t invert,
                                 uint32_t polarity, const int16_t *coeffs, size_t nr_coeffs, struct mfm_runrs_state *state, int16_t *pending,
                                 const struct mfm_gate_run *gate_runs, size_t nr_gate_runs, const int16_t *gate_payload,
                                 size_t nr_gate_elems, struct mfm_runrs_run *runs, size_t max_runs, size_t *nr_runs, uint32_t *bits,
                                 size_t max_words, size_t *nr_words)
{
    if (polarity != MFM_BITS_NEG && polarity != MFM_BITS_POS) {
        return rr_fail(MFM_E_INVAL, "polarity must be MFM_BITS_NEG or MFM_BITS_POS");
    }
    return rr_twin_call(nr_channels, window_samples, interpolate, decimate, invert, coeffs, nr_coeffs, state, pending, gate_runs, nr_gate_runs,
                        gate_payload, nr_gate_elems, runs, max_runs, nr_runs, nullptr, bits, polarity, max_words, nr_words);
}

int mfm_hosttwin_runrs_dc_call(uint32_t nr_channels, double pole, struct mfm_runrs_dc_state *dc, const struct mfm_runrs_run *runs,
                               size_t nr_runs, int16_t *payload, size_t nr_elems)
{
    if (!nr_channels || !dc || (!runs && nr_runs) || (!payload && nr_elems)) {
        return MFM_E_INVAL;
    }
    int32_t p = 0;
    if (!mfm_runrs_dc_pole(pole, &p)) {
        return rr_fail(MFM_E_INVAL, RR_BAD_POLE);
    }
    for (size_t r = 0; r < nr_runs; r++) {
        const mfm_runrs_run &o = runs[r];
        const bool first = r == 0 || runs[r - 1].channel != o.channel;
        if (o.channel >= nr_channels || (r && runs[r - 1].channel > o.channel)) {
            return rr_fail(MFM_E_INVAL, "the run list is not a burst resampler's: a channel does not exist or the channels do not ascend");
        }
        if (!first && 0u == (o.flags & MFM_RUNRS_BEGINS)) {
            return rr_fail(MFM_E_INVAL, "the run list is not a burst resampler's: a run that continues a stretch is not its channel's first");
        }
        if (o.out_offset > nr_elems || o.nr_out > nr_elems - o.out_offset) {
            return rr_fail(MFM_E_INVAL, "the run list is not a burst resampler's: a run's outputs lie beyond the payload");
        }
    }
    for (size_t r = 0; r < nr_runs; r++) {
        const mfm_runrs_run &o = runs[r];
        const bool first = r == 0 || runs[r - 1].channel != o.channel;
        const bool last = r + 1 == nr_runs || runs[r + 1].channel != o.channel;
        mfm_runrs_dc_carry k = mfm_runrs_dc_start(dc + o.channel, first, o.flags);
        int16_t *yy = payload + o.out_offset;
        for (uint32_t i = 0; i < o.nr_out; i++) {
            yy[i] = mfm_runrs_dc_sample(k, p, yy[i]);
        }
        if (last) {
            dc[o.channel] = mfm_runrs_dc_leave(k);
        }
    }
    return MFM_OK;
}

} /* extern "C" */
