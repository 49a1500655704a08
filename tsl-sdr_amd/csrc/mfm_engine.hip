/*
 * mfm_engine.hip - host side of the MI355X multifm channel engine behind include/multifm_hip.h.
 *
 * Owns: the channel set (Q14 taps, rotator tables), two device input staging buffers holding
 * [history tail | new block] contiguously, a small ring of output slots (device + pinned host
 * mirror), the per-channel carry state (rotator index, last filtered sample) and three HIP
 * streams (copy-in, compute, copy-out) so H2D, the fused kernel and D2H of consecutive blocks
 * overlap.  What the reference keeps per channel thread in struct direct_fir / struct
 * multifm_fm_demod (filter/direct_fir.h:9-74, multifm/fm_demod.c:14-18) lives here per engine.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/multifm_hip.h"
#include "mfm_kernel.h"
#include "mfm_numerics.h"
#include "mfm_taps.h"
#include "mfm_plan.h"
#include "mfm_launch_plan.h"
#include "mfm_engine_internal.h"

/* every kernel file exports a pair: select (which template instance runs a launch description: mfm_plan.hip, at commit) and
 * launch (through that pointer) */
extern "C" hipError_t mfm_launch_channel_kernel(const void *kfn, const mfm_launch *L, uint32_t lds_bytes, hipStream_t stream);
extern "C" hipError_t mfm_launch_channel_kernel_mfma(const void *kfn, const mfm_launch_mfma *L, uint32_t lds_bytes,
                                                     uint32_t grid, hipStream_t stream);
extern "C" hipError_t mfm_disc_test_dot2(const int *s_re, const int *s_im, int *pcm, uint32_t n, const float2 *lut, hipStream_t stream);
extern "C" hipError_t mfm_disc_test_mfma(const int *s_re, const int *s_im, int *pcm, uint32_t n, const float2 *lut, hipStream_t stream);
extern "C" hipError_t mfm_disc_test_v3(const int *s_re, const int *s_im, int *pcm, uint32_t n, const float2 *lut, hipStream_t stream);
extern "C" hipError_t mfm_launch_channel_kernel_v3(const void *kfn, const mfm_launch_v3 *L, uint32_t lds_bytes, uint32_t grid,
                                                   hipStream_t stream);


namespace {

thread_local char g_last_error[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                                        \
    do {                                                                                                     \
        hipError_t err_ = (expr);                                                                            \
        if (err_ != hipSuccess) {                                                                            \
            return fail(MFM_E_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(err_), __FILE__,     \
                        __LINE__);                                                                           \
        }                                                                                                    \
    } while (0)

#define MFM_TRY(expr)                                                                                        \
    do {                                                                                                     \
        const int rc_ = (expr);                                                                              \
        if (rc_ != MFM_OK) {                                                                                 \
            return rc_;                                                                                      \
        }                                                                                                    \
    } while (0)

/* a device copy of a host table */
template <class P, class T>
int upload(P **dst, const std::vector<T> &v)
{
    void *d = nullptr;
    HIP_TRY(hipMalloc(&d, v.size() * sizeof(T)));
    *dst = static_cast<P *>(d);
    HIP_TRY(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return MFM_OK;
}

/* FNV-1a of the 257 float bit patterns of the fast_atan2f table */
constexpr uint64_t MFM_ATAN_TABLE_FNV1A = 0x674d1aab1787b44bull;

constexpr int kOutSlots = 4;      /* output ring depth (2 in device-only mode) */
constexpr int kMaxInBufs = 3;     /* input buffers: 2, or 3 when the engine coalesces (mfm_engine_config::coalesce_samples) */
constexpr int kTimingPairs = 256; /* event pairs kept before the oldest is folded into the total */
constexpr uint64_t kSparseTiming = 4; /* MFM_F_TIMING_SPARSE: one launch in this many is bracketed */
constexpr uint64_t kCycleRing = 1024; /* launches whose shader-clock stamps are kept (mfm_engine_get_launch_cycles) */
constexpr size_t kLaunchRing = 4096; /* per-launch durations kept for mfm_engine_get_launch_ms() */

struct OutSlot {
    int16_t *d_pcm = nullptr;
    uint32_t *d_iq = nullptr;
    int16_t *h_pcm = nullptr;
    uint32_t *h_iq = nullptr;
    hipEvent_t ready = nullptr; /* D2H (or, device-only, the kernel) finished */
    uint64_t first_output = 0;
    uint32_t nr_outputs = 0;
    enum { FREE, INFLIGHT, FETCHED } state = FREE;
};

} /* namespace */

struct mfm_engine {
    mfm_engine_config cfg{};
    std::vector<Channel> chans;
    uint32_t nr_taps = 0;
    bool committed = false;
    bool any_iq = false;

    /* which kernel runs and how (mfm_plan.h); at commit its launch descriptions get the device tables below */
    KernelPlan plan;

    /* device tables */
    uint32_t *d_coef = nullptr, *d_tapoff = nullptr;
    uint32_t *d_afrag = nullptr;
    int32_t *d_krow = nullptr;
    int32_t *d_krow8[4] = { nullptr, nullptr, nullptr, nullptr }; /* [MFM_IN_*]: row constants of the 8-bit input forms */
    mfm_chan_info *d_info = nullptr;
    uint2 *d_rot = nullptr;
    float2 *d_lut = nullptr;
    mfm_chan_state *d_state[2] = { nullptr, nullptr };
    uint64_t rot_entries = 0;

    /* input staging: nbuf buffers used in turn, each [history tail | blocks accepted since the last launch] */
    uint32_t *d_in[kMaxInBufs] = { nullptr, nullptr, nullptr };
    bool own_in = false;
    uint32_t *h_in[kMaxInBufs] = { nullptr, nullptr, nullptr }; /* pinned, for push() */
    uint16_t *d_raw[kMaxInBufs] = { nullptr, nullptr, nullptr }; /* push_bytes(): 8-bit IQ pairs as they came off the wire */
    hipEvent_t in_free[kMaxInBufs] = { nullptr, nullptr, nullptr };
    hipEvent_t in_free_wait[kMaxInBufs] = { nullptr, nullptr, nullptr }; /* the end of the launch that last read buffer i:
                                                          in_free[i], or the timing event recorded at the same point of
                                                          the stream.  acquire_input() waits on it, the coalescing policy
                                                          queries it */
    hipStream_t in_free_on[kMaxInBufs] = { nullptr, nullptr, nullptr }; /* the stream in_free_wait[i] was recorded on */
    hipEvent_t in_ready = nullptr;
    int nbuf = 2;     /* 3 with coalesce_samples: one being read, one queued behind it, one being filled */
    int cur_in = 0;
    uint32_t tail = 0; /* unconsumed samples at the front of d_in[cur_in] (behind `hist`): the history the next outputs need */
    uint32_t hist = 0; /* second-generation kernel: already consumed samples kept in front of them - the decimation once the
                          stream has produced an output, 0 before -, from which a launch recomputes the output in front of
                          it instead of reading carried state (mfm_launch_v3::hist) */
    uint32_t pend = 0; /* samples accepted into d_in[cur_in] behind the history and not yet launched (coalesce_samples) */
    uint32_t last_launch_samples = 0; /* what the most recent launch read: a second launch is queued behind one in flight
                                         once a quarter of that has gathered */
    uint64_t submits = 0;
    /* pushes straight out of the caller's pinned memory (mfm_engine_push_pinned): a ticket per push, an event per ticket */
    /* Copies complete in order (one copy stream), so a ticket is through as soon as ANY event recorded behind it is: events
     * are recorded only when somebody asks about a ticket no recorded event covers yet (an event per push cost more host
     * time than the staging copy it replaced), a few of them in rotation. */
    static constexpr uint64_t kCopyRing = 4;
    hipEvent_t copy_ev[kCopyRing] = {};
    uint64_t copy_ev_seq[kCopyRing] = {}; /* the ticket each of them covers (0: not recorded) */
    uint64_t copy_ev_next = 0;
    uint64_t copy_seq = 0, copy_done_seq = 0;
    bool wait_copy_stream = false; /* blocks staged on the engine's copy stream since the last launch: the launch waits for
                                      that stream once, instead of every push recording and waiting for an event */
    int last_launch_buf = -1, last_launch_fmt = MFM_IN_CS16;
    uint32_t last_launch_hist = 0;
    /* 8-bit blocks may sit in the input buffers as they came off the wire (2 bytes per sample, push_bytes): the format of
     * what was staged into each buffer, and of the history at the front of d_in[cur_in] */
    int in_fmt[kMaxInBufs] = { MFM_IN_CS16, MFM_IN_CS16, MFM_IN_CS16 };
    int tail_fmt = MFM_IN_CS16;
    uint16_t *d_tailtmp = nullptr; /* a history kept as bytes is widened through here when an int16 block follows it */
    uint64_t launches_8bit = 0;

    /* outputs */
    OutSlot slots[kOutSlots];
    int nslots = kOutSlots;
    uint64_t submit_seq = 0; /* submits that produced outputs */
    uint64_t fetch_seq = 0;
    int last_slot = -1;

    hipStream_t s_in = nullptr, s_compute = nullptr, s_out = nullptr;
    /* MFM_F_OVERLAP: launches alternate between two compute streams (cs[0] = s_compute).  A launch of the second-generation
     * kernel depends on the one before it through input samples only (mfm_launch_v3::hist, ::k_base), so launch k + 1 fills
     * the workgroup slots launch k's shorter chunks free up instead of waiting for its last tile - and for a dispatch. */
    hipStream_t cs[2] = { nullptr, nullptr };
    uint32_t ncs = 1;
    uint32_t si = 0;              /* index into cs of the next launch */
    hipStream_t s_last = nullptr; /* the stream the most recent launch went to (mfm_engine_stream) */
    hipEvent_t tail_done[kMaxInBufs] = { nullptr, nullptr, nullptr }; /* overlap: the carry out of buffer i has been copied */
    bool tail_pending[kMaxInBufs] = { false, false, false };
    hipEvent_t kernel_done = nullptr;
    /* Two streams without being asked (include/multifm_hip.h, mfm_engine_stream): an engine whose stream nobody has been
     * handed can only be observed through sync / stats, which wait for both streams.  `pinned`: the stream has been handed
     * out (or the engine belongs to a device group) - one stream from then on, unless MFM_F_OVERLAP asks for two. */
    bool auto_alt = false, pinned = false;
    uint64_t overlapped = 0; /* launches that left their carry to the copy below and so did not hold back the next one */
    /* Early carry (int16 blocks on mfm_kernel_v3.hip): when a launch alternates, the next launch's [hist | history tail] is
     * copied at submit time by a one-workgroup kernel on s_in - behind the producer of this block and behind no channel
     * kernel - into a slot of d_ring, and the next launch reads it from there (mfm_launch_v3::head).  Pass r of
     * launch_locked() reads buffer r % nbuf and, if its head is in the ring, slot r % (nbuf + 1).  No event guards a slot:
     * why none is needed stands with the decision, at LaunchPlan::early (mfm_launch_plan.h). */
    uint32_t *d_ring = nullptr;
    uint32_t ring_slot = 0;          /* samples per slot: 2 * D + T + 16 */
    uint64_t pass = 0;               /* launch_locked() passes since the stream's start: buffer pass % nbuf is being filled */
    const uint32_t *head = nullptr;  /* the [hist | tail] of the buffer being filled is here, not at its front ... */
    hipEvent_t head_ev = nullptr;    /* ... once this has happened */
    const uint32_t *last_head = nullptr; /* the most recent launch read its first last_head_n samples from here */
    uint32_t last_head_n = 0;

    /* stream bookkeeping */
    int parity = 0;
    uint64_t samples_in = 0, outputs = 0, launches = 0;
    uint32_t grid_last = 0;

    /* one producer thread (push/submit) and one consumer thread (fetch/release) may use the engine
     * concurrently: this guards the bookkeeping they share; device waits happen outside it */
    std::mutex mu;

    /* timing */
    hipEvent_t t0[kTimingPairs] = {}, t1[kTimingPairs] = {};
    bool timing_events = false;
    uint64_t t_head = 0, t_tail = 0;
    double kernel_ms = 0.0;
    /* MFM_F_TIMING, second-generation kernels: per-launch durations in the shader's own clocks (mfm_launch_v3::cyc) */
    unsigned long long *d_cyc = nullptr; /* [kCycleRing][2] */
    std::vector<float> launch_ms; /* ring of the last kLaunchRing launch durations */
    uint64_t launch_ms_n = 0;     /* durations folded so far */
    /* An event pair around a launch that shares the chip with the one before it measures its wait for workgroup slots: an
     * engine with two compute streams records none, and a timed launch's duration is the kernel's own stamp in d_cyc (100 MHz
     * reference ticks of its longest workgroup).  The 0-based numbers of the timed launches not yet folded, oldest first. */
    std::vector<uint64_t> stamp_pending;
};

namespace {

/* The dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) belongs to a kernel instance on a device, not to an
 * engine: two engines of one process can share an instance with different image sizes (first-generation kernels with
 * different decimations; the generic second-generation instances).  The limit is therefore only ever RAISED: the largest
 * value any engine of the process has asked for, per (device, instance). */
int raise_lds_limit(int device, const void *fn, uint32_t lds)
{
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, uint32_t> limit;
    std::lock_guard<std::mutex> guard(mu);
    uint32_t &have = limit[std::make_pair(device, fn)];
    if (lds > have) {
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        have = lds;
    }
    return MFM_OK;
}

/*
 * The discriminator's division (mfm_numerics.h, mfm_div_unit) is correctly rounded with the reciprocals gfx950's
 * v_rcp_f32 returns - shown for all operands by tools/div_proof.c on the table tools/rcp_check.hip reads off the device.  It
 * would NOT be for every reciprocal within one ulp: 8388608 / 16777215 needs the correctly rounded reciprocal of
 * 2^24 - 1, 13981011 / 16777213 and 15099490 / 16777211 a reciprocal that is not too high.  Once per process and device
 * the engine therefore runs exactly those quotients (all octants, the kernel variant in use) through the device's
 * discriminator and compares with the host twin's IEEE division: a device that answers differently is refused at
 * commit instead of producing PCM that is one LSB off once in 10^7 samples.
 */
/* What v_rcp_f32 returns for every binary32 significand, as one number: the difference (in ulps) between the device's
 * reciprocal of 2^23 + i and the correctly rounded one, hashed with i; the counts of -1 / 0 / +1 / anything else beside it.
 * tools/div_proof.c's enumeration holds for the table this hash stands for (MFM_RCP_TABLE_HASH_GFX950, read off an MI355X
 * by tools/rcp_check.hip: 89 % correctly rounded, 9 % one ulp low, 2 % one ulp high). */
__global__ void mfm_rcp_table_kernel(unsigned long long *acc)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const float b = (float)((1u << 23) + i);
    const float r = __builtin_amdgcn_rcpf(b);
    const float rn = __fdiv_rn(1.0f, b);
    const int32_t d = (int32_t)__float_as_uint(r) - (int32_t)__float_as_uint(rn);
    unsigned long long h = (unsigned long long)(uint32_t)(d + 8) * ((unsigned long long)i * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull);
    for (int o = 32; o > 0; o >>= 1) {
        h += __shfl_down(h, o);
    }
    const unsigned long long lo = __ballot(d == -1), eq = __ballot(d == 0), hi = __ballot(d == 1);
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(&acc[0], h);
        atomicAdd(&acc[1], (unsigned long long)__popcll(lo));
        atomicAdd(&acc[2], (unsigned long long)__popcll(eq));
        atomicAdd(&acc[3], (unsigned long long)__popcll(hi));
        atomicAdd(&acc[4], 64ull - (unsigned long long)(__popcll(lo) + __popcll(eq) + __popcll(hi)));
    }
}

/* the discriminator's division against the IEEE quotient on pseudo-random significand pairs and on the divisors next to a
 * power of two (the classical hard ones): the net under a device whose reciprocal table is not the one of the proof */
__global__ void mfm_div_sweep_kernel(uint32_t seed, uint32_t per_thread, unsigned long long *bad)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t x = ((uint64_t)seed << 32) ^ ((uint64_t)t * 0xD1B54A32D192ED03ull + 0x9E3779B97F4A7C15ull);
    uint32_t wrong = 0;
    for (uint32_t k = 0; k < per_thread; k++) {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        uint32_t A = (1u << 23) | ((uint32_t)x & 0x7fffffu), B = (1u << 23) | ((uint32_t)(x >> 32) & 0x7fffffu);
        if ((k & 3u) == 3u) {
            const uint32_t near = (uint32_t)(x >> 55) & 0xffu; /* divisors within 256 of 2^24 and of 2^23 */
            B = (k & 4u) ? (1u << 24) - 1u - near : (1u << 23) + near;
        }
        const float b = (float)B;
        const float a = A <= B ? (float)A : 0.5f * (float)A;
        wrong += mfm_div_unit(a, b) != __fdiv_rn(a, b) ? 1u : 0u;
    }
    if (wrong) {
        atomicAdd(bad, (unsigned long long)wrong);
    }
}

int rcp_table_read(int device, uint64_t out[5])
{
    HIP_TRY(hipSetDevice(device));
    unsigned long long *d = nullptr;
    HIP_TRY(hipMalloc(&d, 5 * sizeof(unsigned long long)));
    int rc = MFM_OK;
    if (hipMemset(d, 0, 5 * sizeof(unsigned long long)) != hipSuccess) {
        rc = fail(MFM_E_DEVICE, "hipMemset failed");
    } else {
        hipLaunchKernelGGL(mfm_rcp_table_kernel, dim3((1u << 23) / 256u), dim3(256), 0, nullptr, d);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, d, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) {
            rc = fail(MFM_E_DEVICE, "the reciprocal-table kernel failed on device %d", device);
        }
    }
    (void)hipFree(d);
    return rc;
}

int div_sweep(int device, uint64_t *bad, uint64_t *tried)
{
    HIP_TRY(hipSetDevice(device));
    unsigned long long *d = nullptr;
    HIP_TRY(hipMalloc(&d, sizeof(unsigned long long)));
    int rc = MFM_OK;
    const uint32_t blocks = 4096, threads = 256, per_thread = 256; /* 2^28 quotients, a few ms */
    if (hipMemset(d, 0, sizeof(unsigned long long)) != hipSuccess) {
        rc = fail(MFM_E_DEVICE, "hipMemset failed");
    } else {
        hipLaunchKernelGGL(mfm_div_sweep_kernel, dim3(blocks), dim3(threads), 0, nullptr, 0x5eed5eedu, per_thread, d);
        unsigned long long h = 0;
        if (hipGetLastError() != hipSuccess || hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) {
            rc = fail(MFM_E_DEVICE, "the division sweep failed on device %d", device);
        }
        *bad = h;
        *tried = (uint64_t)blocks * threads * per_thread;
    }
    (void)hipFree(d);
    return rc;
}

int division_selftest(int device, int variant)
{
    static std::mutex mu;
    static std::map<std::pair<int, int>, int> done;
    std::lock_guard<std::mutex> guard(mu);
    auto it = done.find(std::make_pair(device, variant));
    if (it != done.end()) {
        return it->second == MFM_OK ? MFM_OK : fail(it->second, "the division self-test failed on device %d before", device);
    }
    static const int32_t pairs[][2] = { { 8388608, 16777215 }, { 13981011, 16777213 }, { 15099490, 16777211 },
                                        { 8388607, 16777215 }, { 12582912, 16777215 }, { 1, 3 }, { 16777215, 16777215 },
                                        { 5, 2147483647 }, { 1073741823, 2147483646 } };
    std::vector<int32_t> re, im;
    for (const auto &p : pairs) {
        for (int o = 0; o < 8; o++) {
            const int32_t x = (o & 1) ? p[0] : p[1], y = (o & 1) ? p[1] : p[0];
            re.push_back((o & 2) ? -x : x);
            im.push_back((o & 4) ? -y : y);
        }
    }
    std::vector<int16_t> got(re.size());
    int rc = mfm_devtest_discriminate(variant, re.data(), im.data(), re.size(), got.data(), device);
    if (rc == MFM_OK) {
        for (size_t i = 0; i < re.size(); i++) {
            const int16_t want = (int16_t)mfm_hosttwin_discriminate(re[i], im[i]);
            if (got[i] != want) {
                rc = fail(MFM_E_DEVICE, "division self-test: discriminator(%d, %d) = %d on device %d, %d by IEEE division - this "
                                        "device's v_rcp_f32 differs from gfx950's (tools/div_proof.c)", re[i], im[i], got[i], device, want);
                break;
            }
        }
    }
    if (rc == MFM_OK) {
        /* once per device: is v_rcp_f32's table the one tools/div_proof.c enumerated?  If it is not (another stepping, other
         * microcode), the three quotients above are no proof: 2^28 quotients against the IEEE division decide, and a
         * single wrong one refuses the device. */
        static std::map<int, int> table_done;
        auto td = table_done.find(device);
        if (td == table_done.end()) {
            uint64_t t[5] = { 0, 0, 0, 0, 0 };
            int trc = rcp_table_read(device, t);
            if (trc == MFM_OK && t[0] != MFM_RCP_TABLE_HASH_GFX950) {
                uint64_t bad = 0, tried = 0;
                trc = div_sweep(device, &bad, &tried);
                if (trc == MFM_OK && bad != 0) {
                    trc = fail(MFM_E_DEVICE, "device %d: v_rcp_f32 is not gfx950's table (hash %016llx, %llu / %llu / %llu one ulp low / exact / "
                                             "high) and %llu of %llu quotients differ from the IEEE division", device,
                               (unsigned long long)t[0], (unsigned long long)t[1], (unsigned long long)t[2], (unsigned long long)t[3],
                               (unsigned long long)bad, (unsigned long long)tried);
                }
            }
            table_done[device] = trc;
            rc = trc;
        } else if (td->second != MFM_OK) {
            rc = fail(td->second, "the reciprocal-table check failed on device %d before", device);
        }
    }
    done[std::make_pair(device, variant)] = rc;
    return rc;
}


void fold_duration(mfm_engine *e, float ms)
{
    e->kernel_ms += ms;
    if (e->launch_ms.size() < kLaunchRing) {
        e->launch_ms.resize(kLaunchRing);
    }
    e->launch_ms[e->launch_ms_n % kLaunchRing] = ms;
    e->launch_ms_n++;
}

/* the stamps of the timed launches of a two-stream engine (mfm_engine::stamp_pending).  all: every one of them, after waiting
 * for the compute streams; else those of launches that are known to have ended - a launch eight launches back has, since
 * acquire_input() waits for the launch nbuf passes back.  A stamp that has left the readable half of the ring (its slot is
 * zeroed by the launch kCycleRing / 2 behind its own) is dropped: that launch is not counted as timed. */
int fold_stamps(mfm_engine *e, bool all)
{
    if (e->stamp_pending.empty() || !e->d_cyc) {
        e->stamp_pending.clear();
        return MFM_OK;
    }
    if (all) {
        HIP_TRY(hipStreamSynchronize(e->cs[0]));
        if (e->cs[1] != e->cs[0]) {
            HIP_TRY(hipStreamSynchronize(e->cs[1]));
        }
    }
    std::vector<unsigned long long> ring(kCycleRing * 2);
    HIP_TRY(hipMemcpy(ring.data(), e->d_cyc, ring.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    size_t done = 0;
    for (; done < e->stamp_pending.size(); done++) {
        const uint64_t seq = e->stamp_pending[done];
        if (!all && seq + 8u > e->launches) {
            break;
        }
        const uint64_t tag = ((seq + 1u) & 0xffffffu) << 40, mask = (1ull << 40) - 1ull;
        const unsigned long long b = ring[2 * (seq % kCycleRing) + 1];
        if (seq + kCycleRing / 2u >= e->launches && (b & ~mask) == tag) {
            fold_duration(e, (float)((double)(b & mask) / 1e5));
        }
    }
    e->stamp_pending.erase(e->stamp_pending.begin(), e->stamp_pending.begin() + (ptrdiff_t)done);
    return MFM_OK;
}

int fold_timing(mfm_engine *e, bool all)
{
    /* (stamps are older than event pairs: an engine goes from two streams to one - when it is pinned - and never back) */
    if (all || (!e->stamp_pending.empty() && e->launches - e->stamp_pending.front() >= kCycleRing / 4u)) {
        MFM_TRY(fold_stamps(e, all));
    }
    while (e->t_tail < e->t_head && (all || e->t_head - e->t_tail >= (uint64_t)kTimingPairs)) {
        const int i = (int)(e->t_tail % kTimingPairs);
        HIP_TRY(hipEventSynchronize(e->t1[i]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e->t0[i], e->t1[i]));
        fold_duration(e, ms);
        e->t_tail++;
    }
    return MFM_OK;
}

template <class P>
void free_dev(P *&p)
{
    (void)hipFree(p);
    p = nullptr;
}

template <class P>
void free_host(P *&p)
{
    if (p) {
        (void)hipHostFree(p);
    }
    p = nullptr;
}

void free_event(hipEvent_t &ev)
{
    if (ev) {
        (void)hipEventDestroy(ev);
    }
    ev = nullptr;
}

void free_stream(hipStream_t &s)
{
    if (s) {
        (void)hipStreamDestroy(s);
    }
    s = nullptr;
}

void free_device(mfm_engine *e)
{
    if (!e->committed) {
        return;
    }
    (void)hipSetDevice(e->cfg.device);
    (void)hipDeviceSynchronize();
    free_dev(e->d_coef);
    free_dev(e->d_tapoff);
    free_dev(e->d_afrag);
    free_dev(e->d_krow);
    for (int32_t *&k : e->d_krow8) {
        free_dev(k);
    }
    free_dev(e->d_tailtmp);
    free_dev(e->d_info);
    free_dev(e->d_rot);
    free_dev(e->d_cyc);
    free_dev(e->d_ring);
    e->head = e->last_head = nullptr;
    e->head_ev = nullptr; /* (one of tail_done[]) */
    e->last_head_n = 0;
    e->stamp_pending.clear();
    free_dev(e->d_lut);
    for (mfm_chan_state *&s : e->d_state) {
        free_dev(s);
    }
    for (int i = 0; i < kMaxInBufs; i++) {
        if (e->own_in) {
            (void)hipFree(e->d_in[i]);
        }
        e->d_in[i] = nullptr;
        free_dev(e->d_raw[i]);
        free_host(e->h_in[i]);
        free_event(e->in_free[i]);
        e->in_free_wait[i] = nullptr; /* (in_free[i] or a timing event) */
        free_event(e->tail_done[i]);
        e->tail_pending[i] = false;
    }
    for (OutSlot &s : e->slots) {
        free_dev(s.d_pcm);
        free_dev(s.d_iq);
        free_host(s.h_pcm);
        free_host(s.h_iq);
        free_event(s.ready);
        s = OutSlot();
    }
    for (int i = 0; i < kTimingPairs; i++) {
        free_event(e->t0[i]);
        free_event(e->t1[i]);
    }
    e->timing_events = false;
    for (uint64_t i = 0; i < mfm_engine::kCopyRing; i++) {
        free_event(e->copy_ev[i]);
        e->copy_ev_seq[i] = 0;
    }
    e->copy_seq = e->copy_done_seq = e->copy_ev_next = 0;
    e->wait_copy_stream = false;
    free_event(e->in_ready);
    free_event(e->kernel_done);
    if (e->cs[1] != e->s_compute) {
        free_stream(e->cs[1]);
    }
    e->cs[0] = e->cs[1] = e->s_last = nullptr;
    free_stream(e->s_in);
    free_stream(e->s_compute);
    free_stream(e->s_out);
    e->committed = false;
}

int write_state_fresh(mfm_engine *e)
{
    std::vector<mfm_chan_state> st(e->plan.ngroups * MFM_CG);
    for (auto &s : st) {
        s.carry_q = 0; /* fm_demod.c: last sample starts at 0 (TZAALLOC, :29) */
        s.kb = 0;
    }
    for (int i = 0; i < 2; i++) {
        HIP_TRY(hipMemcpy(e->d_state[i], st.data(), st.size() * sizeof(mfm_chan_state), hipMemcpyHostToDevice));
    }
    e->parity = 0;
    return MFM_OK;
}

/*
 * 8-bit ingest on the device.  The reference widens 8-bit captures to int16 on the
 * host before anything else sees them: cs8 is a plain sign extension (multifm/file_if.c:91-103); cu8 reads the
 * bytes as SIGNED and subtracts 127 (:122,:139-151; after an odd number of samples the last one misses the
 * subtraction, :146-150); the RTL-SDR front end computes (u8 - 127) << 7 (multifm/rtl_sdr_if.c:146-158).
 * Here the raw byte pairs cross PCIe (half the bytes) and are widened where the channel kernel will read them.
 * HBM-bound: 2 bytes in, 4 bytes out per sample; one lane handles 8 samples (16 B in, 2 x 16 B out).
 */
__device__ __forceinline__ uint32_t mfm_widen_pair(uint32_t two_bytes, int format)
{
    int32_t a, b;
    if (format == MFM_IN_RTLSDR_U8) {
        a = (((int32_t)(two_bytes & 0xffu)) - 127) * 128;
        b = (((int32_t)((two_bytes >> 8) & 0xffu)) - 127) * 128;
    } else {
        a = (int8_t)(two_bytes & 0xffu);
        b = (int8_t)((two_bytes >> 8) & 0xffu);
        if (format == MFM_IN_CU8) {
            a -= 127;
            b -= 127;
        }
    }
    return mfm_pack16(a, b);
}

__global__ __launch_bounds__(256) void mfm_unpack_kernel(const uint16_t *raw, uint32_t *dst, uint32_t nr_samples, int format,
                                                         int cu8_odd_tail)
{
    const uint32_t ngroups = nr_samples / 8;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += gridDim.x * blockDim.x) {
        const uint4 v = reinterpret_cast<const uint4 *>(raw)[g];
        const uint32_t w[4] = { v.x, v.y, v.z, v.w };
        uint32_t o[8];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            o[2 * k] = mfm_widen_pair(w[k] & 0xffffu, format);
            o[2 * k + 1] = mfm_widen_pair(w[k] >> 16, format);
        }
        reinterpret_cast<uint4 *>(dst)[2 * g] = make_uint4(o[0], o[1], o[2], o[3]);
        reinterpret_cast<uint4 *>(dst)[2 * g + 1] = make_uint4(o[4], o[5], o[6], o[7]);
    }
    /* the last nr_samples % 8, one lane each */
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t s = ngroups * 8 + t;
    if (s < nr_samples) {
        uint32_t out = mfm_widen_pair(raw[s], format);
        if (cu8_odd_tail && format == MFM_IN_CU8 && (nr_samples & 1u) && s == nr_samples - 1) {
            const uint32_t two = raw[s]; /* file_if.c:146-150: the remainder loop stores the bare cast */
            out = mfm_pack16((int8_t)(two & 0xffu), (int8_t)(two >> 8));
        }
        dst[s] = out;
    }
}

/* The early carry's copy (mfm_engine::d_ring) and its way back to a buffer's front: n samples - about a kilobyte -, one
 * workgroup, no LDS, a few registers, so that it finds a place on a chip whose every SIMD is full of channel-kernel waves as
 * soon as one of them leaves.  (A hipMemcpyAsync is a shader copy as well, with a dispatch and a barrier packet around it.) */
__global__ __launch_bounds__(256) void mfm_carry_kernel(const uint32_t *src, uint32_t *dst, uint32_t n)
{
    for (uint32_t i = threadIdx.x; i < n; i += 256u) {
        dst[i] = src[i];
    }
}

} /* namespace */

/* ------------------------------------------------------------------------------------- */

extern "C" {

const char *mfm_strerror(int err)
{
    switch (err) {
    case MFM_OK: return "ok";
    case MFM_E_INVAL: return "invalid argument";
    case MFM_E_NOMEM: return "out of memory";
    case MFM_E_BUSY: return "busy";
    case MFM_E_DEVICE: return "HIP device error";
    case MFM_E_STATE: return "invalid state";
    case MFM_E_DONE: return "done";
    default: return "unknown error";
    }
}

const char *mfm_last_error(void)
{
    return g_last_error;
}

/* for the other translation units of the library (mfm_resampler.hip, mfm_pocsag.hip) */
__attribute__((visibility("hidden"))) void mfm_internal_set_error(const char *msg)
{
    snprintf(g_last_error, sizeof(g_last_error), "%s", msg);
}

size_t mfm_engine_input_bytes(uint32_t max_block_samples, uint32_t nr_taps)
{
    return (size_t)input_capacity(max_block_samples, 0, nr_taps) * sizeof(uint32_t);
}

size_t mfm_engine_input_bytes_cfg(const struct mfm_engine_config *cfg, uint32_t nr_taps, uint32_t *nr_buffers)
{
    if (!cfg) {
        return 0;
    }
    if (nr_buffers) {
        *nr_buffers = cfg->coalesce_samples ? 3u : 2u;
    }
    return (size_t)input_capacity(cfg->max_block_samples, cfg->coalesce_samples, nr_taps) * sizeof(uint32_t);
}

int mfm_engine_create(struct mfm_engine **pe, const struct mfm_engine_config *cfg)
{
    if (!pe || !cfg) {
        return fail(MFM_E_INVAL, "NULL argument");
    }
    *pe = nullptr;
    if (cfg->abi_version != MFM_ABI_VERSION) {
        return fail(MFM_E_INVAL, "ABI version %u, library is %u", cfg->abi_version, MFM_ABI_VERSION);
    }
    if (0 == cfg->decimation || 0 == cfg->sample_rate_hz || 0 == cfg->max_block_samples) {
        return fail(MFM_E_INVAL, "decimation, sample rate and max block must be non-zero");
    }
    if (cfg->max_block_samples > (1u << 30)) {
        return fail(MFM_E_INVAL, "max_block_samples %u too large", cfg->max_block_samples);
    }
    if ((cfg->ext_input[0] == nullptr) != (cfg->ext_input[1] == nullptr) ||
        (cfg->coalesce_samples && (cfg->ext_input[0] == nullptr) != (cfg->ext_input[2] == nullptr))) {
        return fail(MFM_E_INVAL, "ext_input needs every buffer (two; three with coalesce_samples) or none");
    }
    if ((uint64_t)cfg->max_block_samples + cfg->coalesce_samples > (1u << 30)) {
        return fail(MFM_E_INVAL, "max_block_samples + coalesce_samples = %llu too large",
                    (unsigned long long)cfg->max_block_samples + cfg->coalesce_samples);
    }
    mfm_engine *e = new (std::nothrow) mfm_engine();
    if (!e) {
        return fail(MFM_E_NOMEM, "engine allocation failed");
    }
    e->cfg = *cfg;
    *pe = e;
    return MFM_OK;
}

void mfm_engine_destroy(struct mfm_engine **pe)
{
    if (!pe || !*pe) {
        return;
    }
    free_device(*pe);
    delete *pe;
    *pe = nullptr;
}

int mfm_engine_add_channel_q14(struct mfm_engine *e, const int16_t *coeff_re, const int16_t *coeff_im,
                               size_t nr_taps, int16_t rot_incr_re, int16_t rot_incr_im, int want_iq)
{
    if (!e || !coeff_re || !coeff_im || 0 == nr_taps) {
        return fail(MFM_E_INVAL, "NULL or empty taps");
    }
    if (e->committed) {
        return fail(MFM_E_STATE, "channel set is frozen after commit");
    }
    if (!e->chans.empty() && nr_taps != e->nr_taps) {
        return fail(MFM_E_INVAL, "all channels share one tap count (%u), got %zu", e->nr_taps, nr_taps);
    }
    if (nr_taps < e->cfg.decimation) {
        /* the reference dereferences a NULL sb_active in this configuration (direct_fir.c:394-398) */
        return fail(MFM_E_INVAL, "taps (%zu) < decimation (%u) is not a valid multifm configuration", nr_taps,
                    e->cfg.decimation);
    }
    if (nr_taps > 65535) {
        return fail(MFM_E_INVAL, "too many taps");
    }
    for (size_t i = 0; i < nr_taps; i++) {
        if (coeff_im[i] == INT16_MIN) {
            /* -ci is not an int16: the packed (cr,-ci) operand cannot hold it */
            return fail(MFM_E_INVAL, "imaginary tap %zu is -32768 (a tap of magnitude 2.0); not supported", i);
        }
    }
    Channel c;
    c.cre.assign(coeff_re, coeff_re + nr_taps);
    c.cim.assign(coeff_im, coeff_im + nr_taps);
    c.incr_re = rot_incr_re;
    c.incr_im = rot_incr_im;
    c.want_iq = want_iq != 0;
    e->nr_taps = (uint32_t)nr_taps;
    e->chans.push_back(std::move(c));
    return (int)e->chans.size() - 1;
}

int mfm_engine_add_channel(struct mfm_engine *e, int32_t offset_hz, const double *lpf_taps, size_t nr_taps,
                           double channel_gain, int want_iq)
{
    if (!e || !lpf_taps || 0 == nr_taps) {
        return fail(MFM_E_INVAL, "NULL or empty taps");
    }
    std::vector<int16_t> cre(nr_taps), cim(nr_taps);
    int16_t ir = 0, ii = 0;
    mfm_taps_rotate_q14(lpf_taps, nr_taps, offset_hz, e->cfg.sample_rate_hz, channel_gain, cre.data(), cim.data());
    mfm_taps_rot_increment(offset_hz, e->cfg.sample_rate_hz, e->cfg.decimation, &ir, &ii);
    return mfm_engine_add_channel_q14(e, cre.data(), cim.data(), nr_taps, ir, ii, want_iq);
}

int mfm_engine_get_channel(struct mfm_engine *e, uint32_t chan, int16_t *coeff_re, int16_t *coeff_im,
                           int16_t rot_incr[2])
{
    if (!e || chan >= e->chans.size()) {
        return fail(MFM_E_INVAL, "no such channel");
    }
    const Channel &c = e->chans[chan];
    if (coeff_re) {
        memcpy(coeff_re, c.cre.data(), c.cre.size() * sizeof(int16_t));
    }
    if (coeff_im) {
        memcpy(coeff_im, c.cim.data(), c.cim.size() * sizeof(int16_t));
    }
    if (rot_incr) {
        rot_incr[0] = c.incr_re;
        rot_incr[1] = c.incr_im;
    }
    return MFM_OK;
}

static int commit_locked(struct mfm_engine *e);

int mfm_engine_commit(struct mfm_engine *e)
{
    if (!e) {
        return fail(MFM_E_INVAL, "NULL engine");
    }
    if (e->committed) {
        return fail(MFM_E_STATE, "already committed");
    }
    for (int i = 0; i < kMaxInBufs; i++) {
        if (e->cfg.ext_input[i] && (reinterpret_cast<uintptr_t>(e->cfg.ext_input[i]) & 15u)) {
            return fail(MFM_E_INVAL, "ext_input buffers must be 16-byte aligned");
        }
    }
    const int rc = commit_locked(e);
    if (rc != MFM_OK && e->committed) {
        /* a failure half-way through the device allocations: release what exists and leave the engine
         * uncommitted (the data-path entry points check `committed`), keeping the failure's message */
        char keep[sizeof(g_last_error)];
        memcpy(keep, g_last_error, sizeof(keep));
        free_device(e);
        memcpy(g_last_error, keep, sizeof(keep));
    }
    return rc;
}

/* Device setup for the plan (mfm_plan.h): the device check, the plan and its host tables, streams and events, the uploads,
 * input buffers and output slots, the launch descriptions' device pointers and each instance's LDS limit. */
static int commit_locked(struct mfm_engine *e)
{
    if (e->chans.empty()) {
        return fail(MFM_E_INVAL, "no channels");
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        return fail(MFM_E_DEVICE, "no HIP device available (this library has no CPU path)");
    }
    if (e->cfg.device < 0 || e->cfg.device >= ndev) {
        return fail(MFM_E_DEVICE, "device %d out of range (%d devices)", e->cfg.device, ndev);
    }
    HIP_TRY(hipSetDevice(e->cfg.device));

    KernelPlan &p = e->plan;
    HostTables t;
    MFM_TRY(plan_channel_kernel(e->cfg, e->chans, e->nr_taps, p));
    MFM_TRY(build_host_tables(p, e->chans, t));
    const bool v3 = 2u == p.variant, dev_only = (e->cfg.flags & MFM_F_DEVICE_ONLY) != 0;
    e->nbuf = e->cfg.coalesce_samples ? 3 : 2;
    e->rot_entries = t.rot.size() + t.rot4.size();

    /* ---- device allocations ---- */
    e->committed = true; /* from here free_device() releases whatever was allocated */
    HIP_TRY(hipStreamCreateWithFlags(&e->s_in, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&e->s_compute, hipStreamNonBlocking));
    e->cs[0] = e->cs[1] = e->s_last = e->s_compute;
    e->ncs = 1;
    e->si = 0;
    e->pinned = false;
    e->overlapped = 0;
    e->pass = 0;
    /* int16 blocks run on mfm_kernel_v3.hip (not the long-filter file): the early carry applies */
    const bool v3s = v3 && p.fmt[MFM_IN_CS16].kfn && p.fmt[MFM_IN_CS16].V.layout != 3u;
    /* two streams by itself: where nobody can tell (the stream has not been handed out: mfm_engine_stream) and the other
     * conditions of include/multifm_hip.h hold; the per-launch ones are launch_plan()'s (mfm_launch_plan.h) */
    e->auto_alt = v3s && dev_only && 2 == e->nbuf && !(e->cfg.flags & MFM_F_OVERLAP);
    if (((e->cfg.flags & MFM_F_OVERLAP) && v3) || e->auto_alt) {
        HIP_TRY(hipStreamCreateWithFlags(&e->cs[1], hipStreamNonBlocking));
        e->ncs = 2;
        for (int i = 0; i < kMaxInBufs; i++) {
            HIP_TRY(hipEventCreateWithFlags(&e->tail_done[i], hipEventDisableTiming));
        }
        if (v3s) {
            e->ring_slot = 2u * p.D + p.T + 16u;
            HIP_TRY(hipMalloc(&e->d_ring, (size_t)(e->nbuf + 1) * e->ring_slot * sizeof(uint32_t)));
        }
    }
    /* (the process has few hardware queues, and streams that share one serialise: a device-only engine copies nothing out) */
    if (!dev_only) {
        HIP_TRY(hipStreamCreateWithFlags(&e->s_out, hipStreamNonBlocking));
    }
    HIP_TRY(hipEventCreateWithFlags(&e->in_ready, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&e->kernel_done, hipEventDisableTiming));

    MFM_TRY(upload(&e->d_coef, t.coef));
    MFM_TRY(upload(&e->d_tapoff, t.tapoff));
    if (p.variant >= 1u) {
        MFM_TRY(upload(&e->d_afrag, t.afrag));
        MFM_TRY(upload(&e->d_krow, t.krow));
    }
    if (p.raw8_ok) {
        for (int fmt = MFM_IN_CS8; fmt <= MFM_IN_RTLSDR_U8; fmt++) {
            MFM_TRY(upload(&e->d_krow8[fmt], t.krow8[fmt]));
        }
        HIP_TRY(hipMalloc(&e->d_tailtmp, ((size_t)p.T + p.D + 16u) * 2u));
    }
    MFM_TRY(upload(&e->d_info, t.info));
    MFM_TRY(t.rot4.empty() ? upload(&e->d_rot, t.rot) : upload(&e->d_rot, t.rot4));
    MFM_TRY(upload(&e->d_lut, t.lut));
    for (int i = 0; i < 2; i++) {
        HIP_TRY(hipMalloc(&e->d_state[i], t.info.size() * sizeof(mfm_chan_state)));
    }
    MFM_TRY(write_state_fresh(e));

    const size_t in_bytes = (size_t)p.cap_in * 4;
    e->own_in = e->cfg.ext_input[0] == nullptr;
    for (int i = 0; i < e->nbuf; i++) {
        if (e->own_in) {
            HIP_TRY(hipMalloc(&e->d_in[i], in_bytes));
        } else {
            e->d_in[i] = static_cast<uint32_t *>(e->cfg.ext_input[i]);
        }
        HIP_TRY(hipEventCreateWithFlags(&e->in_free[i], hipEventDisableTiming));
    }

    e->nslots = dev_only ? 2 : kOutSlots;
    for (int i = 0; i < e->nslots; i++) {
        OutSlot &s = e->slots[i];
        const size_t pcm_bytes = (size_t)p.C * p.out_stride * sizeof(int16_t);
        /* + a dump slot per lane behind the last channel row: the MFMA kernel stores unconditionally and sends
         * what is not an output there */
        HIP_TRY(hipMalloc(&s.d_pcm, pcm_bytes + 64 * sizeof(int16_t)));
        if (p.any_iq) {
            HIP_TRY(hipMalloc(&s.d_iq, pcm_bytes * 2 + 64 * sizeof(uint32_t)));
        }
        if (!dev_only) {
            HIP_TRY(hipHostMalloc(&s.h_pcm, pcm_bytes, hipHostMallocDefault));
            if (p.any_iq) {
                HIP_TRY(hipHostMalloc(&s.h_iq, pcm_bytes * 2, hipHostMallocDefault));
            }
        }
        HIP_TRY(hipEventCreateWithFlags(&s.ready, hipEventDisableTiming));
    }
    if ((e->cfg.flags & MFM_F_TIMING) && v3) {
        HIP_TRY(hipMalloc(&e->d_cyc, kCycleRing * 2 * sizeof(unsigned long long)));
        HIP_TRY(hipMemset(e->d_cyc, 0, kCycleRing * 2 * sizeof(unsigned long long)));
    }
    if (e->cfg.flags & MFM_F_TIMING) {
        e->timing_events = true;
        for (int i = 0; i < kTimingPairs; i++) {
            HIP_TRY(hipEventCreate(&e->t0[i]));
            HIP_TRY(hipEventCreate(&e->t1[i]));
        }
    }

    /* the launch descriptions get the device tables; the instance of each format its LDS limit (on this device, once) */
    for (int fmt = MFM_IN_CS16; fmt <= MFM_IN_RTLSDR_U8; fmt++) {
        FormatPlan &f = p.fmt[fmt];
        const int32_t *krow = fmt == MFM_IN_CS16 ? e->d_krow : e->d_krow8[fmt];
        f.L.coef = e->d_coef;
        f.L.tapoff = e->d_tapoff;
        f.M.afrag = f.V.afrag = e->d_afrag;
        f.M.krow = f.V.krow = krow;
        f.L.info = f.M.info = f.V.info = e->d_info;
        f.L.rot = f.M.rot = e->d_rot;
        f.V.rot = e->d_rot;
        f.L.lut = f.M.lut = f.V.lut = e->d_lut;
        if (f.kfn) {
            MFM_TRY(raise_lds_limit(e->cfg.device, f.kfn, f.lds_bytes));
        }
    }
    MFM_TRY(division_selftest(e->cfg.device, (int)p.variant));
    HIP_TRY(hipDeviceSynchronize());
    return MFM_OK;
}

/* ---- the data path: accept blocks into the buffer being filled, launch it ---- */

} /* extern "C" */

namespace {

/* format of what the buffer being filled holds ([history | accepted blocks]); -1 = nothing, any format can start it */
int buffer_format(const mfm_engine *e)
{
    if (e->pend) {
        return e->in_fmt[e->cur_in];
    }
    return (e->hist + e->tail) ? e->tail_fmt : -1;
}

bool event_done(hipEvent_t ev)
{
    if (!ev) {
        return true;
    }
    if (hipEventQuery(ev) == hipErrorNotReady) {
        (void)hipGetLastError(); /* "not ready" must not surface in somebody's hipGetLastError() check */
        return false;
    }
    return true;
}

/* launches queued or running: 0, 1, or 2 for "two or more".  The launch before the one that last read buffer b ended
 * before it (one compute stream, in order). */
int launches_in_flight(mfm_engine *e)
{
    const int b1 = (e->cur_in + e->nbuf - 1) % e->nbuf, b2 = (e->cur_in + e->nbuf - 2) % e->nbuf;
    if (event_done(e->in_free_wait[b1])) {
        return 0;
    }
    if (b2 == e->cur_in) {
        return 1; /* two buffers: acquire_input() waited for the launch before that one */
    }
    return event_done(e->in_free_wait[b2]) ? 1 : 2;
}

struct SubmitPlan {
    bool must; /* the buffer has to be launched once this block is in (no coalescing, or coalesce_samples gathered) */
    bool may;  /* a launch would find a free output slot */
    bool want; /* the policy of mfm_engine_config::coalesce_samples would launch now although it does not have to */
    uint32_t n_new;
};

/* what accepting nr_samples more (0: what is there) would mean.  Takes the lock for the slot's state. */
void plan_block(mfm_engine *e, size_t nr_samples, SubmitPlan *p, bool locked)
{
    const AcceptPlan a = accept_plan(e->nr_taps, e->cfg.decimation, e->tail, e->pend, nr_samples, e->cfg.coalesce_samples,
                                     (e->cfg.flags & MFM_F_GATHER) != 0);
    p->n_new = a.n_new;
    p->must = a.must;
    if (e->cfg.flags & MFM_F_DEVICE_ONLY) {
        p->may = true;
    } else if (locked) {
        p->may = 0 == p->n_new || e->slots[e->submit_seq % e->nslots].state == OutSlot::FREE;
    } else {
        std::lock_guard<std::mutex> guard(e->mu);
        p->may = 0 == p->n_new || e->slots[e->submit_seq % e->nslots].state == OutSlot::FREE;
    }
    /* (the launches in flight are asked for - event queries - only where the policy has a say) */
    p->want = a.policy && accept_wants(a, launches_in_flight(e), e->last_launch_samples);
}

static_assert(LP_V3_OT == MFM_V3_OT && LP_V3_LEAD == MFM_V3_LEAD, "mfm_launch_plan.h restates mfm_kernel.h's tile");

/* what launch_plan() decides a pass over d_in[cur_in] from */
LaunchInput launch_input(const mfm_engine *e)
{
    const int fmt = e->in_fmt[e->cur_in];
    const FormatPlan &f = e->plan.fmt[fmt];
    LaunchInput in;
    in.T = e->nr_taps;
    in.D = e->cfg.decimation;
    in.variant = e->plan.variant;
    in.raw8 = fmt != MFM_IN_CS16;
    in.hist = e->hist;
    in.tail = e->tail;
    in.pend = e->pend;
    in.ncs = e->ncs;
    in.auto_alt = e->auto_alt;
    in.ring = e->d_ring != nullptr;
    in.head = e->head != nullptr;
    in.alt_wg_per_cu = e->plan.v_wg_per_cu;
    in.wg_per_cu = f.wg_per_cu;
    in.nslices = 2u == in.variant ? f.V.nslices : 1u == in.variant ? f.M.nslices : f.L.nslices;
    in.opl = (uint32_t)e->plan.opl;
    in.ot = f.M.ot;
    return in;
}

/* The channel kernel of a launch with outputs, on S, into `slot`.  *timing_end: the event that stamps its end, if it has one. */
int queue_kernel(mfm_engine *e, const LaunchPlan &lp, const FormatPlan &f, OutSlot *slot, hipStream_t S, hipEvent_t *timing_end)
{
    const int cur = e->cur_in, nxt = (cur + 1) % e->nbuf;
    mfm_chan_state *const st_in = e->d_state[e->parity], *const st_out = e->d_state[e->parity ^ 1];
    uint32_t *const iq_dbg = e->plan.any_iq ? slot->d_iq : nullptr;
    if (!(e->cfg.flags & MFM_F_DEVICE_ONLY)) {
        /* the previous D2H out of this slot must have drained before the kernel rewrites it */
        HIP_TRY(hipStreamWaitEvent(S, slot->ready, 0));
    }
    /* MFM_F_TIMING_SPARSE: every fourth launch carries the event pair.  An event record is a packet the command
     * processor handles between two kernels (~4 us each on MI355X): bracketing every launch of a back-to-back
     * stream costs 6 % of a 0.12 ms step, a sample of them costs under 1 % and measures the same kernel. */
    const bool timed = (e->cfg.flags & MFM_F_TIMING) != 0 &&
                       (!(e->cfg.flags & MFM_F_TIMING_SPARSE) || (e->launches % kSparseTiming) == 0);
    /* two compute streams: no event pairs - a pair around a launch that shares the chip with the one before it measures
     * its wait for slots -, the kernel's own stamp is the duration (mfm_engine::stamp_pending) */
    const bool stamped = timed && e->ncs > 1u && e->d_cyc != nullptr;
    const bool timing = timed && e->ncs <= 1u;
    int ti = 0;
    if (timed) {
        int rc = fold_timing(e, false);
        if (rc != MFM_OK) {
            return rc;
        }
    }
    if (stamped) {
        e->stamp_pending.push_back(e->launches);
    }
    if (timing) {
        ti = (int)(e->t_head % kTimingPairs);
        HIP_TRY(hipEventRecord(e->t0[ti], S));
    }
    if (e->in_fmt[cur] != MFM_IN_CS16) {
        e->launches_8bit++; /* (8-bit blocks stay bytes on the matrix kernels only) */
    }
    e->grid_last = lp.grid;
    if (2u == e->plan.variant) {
        mfm_launch_v3 V = f.V;
        V.x = e->d_in[cur];
        V.n_avail = lp.n_avail;
        V.n_new = lp.n_new;
        V.hist = e->hist;
        V.k_base = e->outputs;
        V.ntiles = lp.ntiles;
        V.nchunks = lp.nchunks;
        V.cl = lp.cl;
        V.nitems = lp.nitems;
        V.tail_src = lp.tail_src;
        V.tail_n = lp.tail_n;
        V.tail_dst = e->d_in[nxt];
        if (lp.two) {
            e->overlapped++;
        }
        if (LP_HEAD_KERNEL == lp.head) {
            V.head = e->head;
            V.head_n = lp.head_n;
        }
        V.pcm = slot->d_pcm;
        V.iq_dbg = iq_dbg;
        if (e->d_cyc) {
            V.cyc = e->d_cyc + 2u * (e->launches % kCycleRing);
            V.cyc_tag = (uint32_t)((e->launches + 1u) & 0xffffffu);
            /* ... and zeroes the slot half a ring ahead, long before that launch folds its maxima into it: a slot never
             * holds an older launch's stamp when its turn comes, whatever the 24-bit tags compare like after 2^24 launches */
            V.cyc_clear = e->d_cyc + 2u * ((e->launches + kCycleRing / 2u) % kCycleRing);
        }
        HIP_TRY(mfm_launch_channel_kernel_v3(f.kfn, &V, f.lds_bytes, lp.grid, S));
    } else if (1u == e->plan.variant) {
        mfm_launch_mfma M = f.M;
        M.x = e->d_in[cur];
        M.n_avail = lp.n_avail;
        M.n_new = lp.n_new;
        M.ntiles = lp.ntiles;
        M.nitems = lp.nitems;
        M.tail_src = lp.tail_src;
        M.tail_n = lp.tail_n;
        M.tail_dst = e->d_in[nxt];
        M.st_in = st_in;
        M.st_out = st_out;
        M.pcm = slot->d_pcm;
        M.iq_dbg = iq_dbg;
        HIP_TRY(mfm_launch_channel_kernel_mfma(f.kfn, &M, f.lds_bytes, lp.grid, S));
    } else {
        mfm_launch L = f.L;
        L.x = e->d_in[cur];
        L.n_avail = lp.n_avail;
        L.n_new = lp.n_new;
        L.ntiles = lp.ntiles;
        L.st_in = st_in;
        L.st_out = st_out;
        L.pcm = slot->d_pcm;
        L.iq_dbg = iq_dbg;
        HIP_TRY(mfm_launch_channel_kernel(f.kfn, &L, f.lds_bytes, S));
    }
    if (timing) {
        HIP_TRY(hipEventRecord(e->t1[ti], S));
        *timing_end = e->t1[ti];
        e->t_head++;
    }
    e->parity ^= 1;
    e->launches++;
    return MFM_OK;
}

/* The next launch's [hist | history tail], where the kernel has not taken it along: into the next pass's ring slot on s_in, or
 * to the front of the next buffer on S_after, the stream of the next launch. */
int queue_carry(mfm_engine *e, const LaunchPlan &lp, hipStream_t S_after)
{
    const int cur = e->cur_in, nxt = (cur + 1) % e->nbuf;
    if (LP_CARRY_RING == lp.carrier) {
        /* the slot: see LaunchPlan::early for why nobody reads it any more */
        uint32_t *const dst = e->d_ring + (size_t)((e->pass + 1u) % (uint64_t)(e->nbuf + 1)) * e->ring_slot;
        if (lp.carry_n > e->ring_slot) {
            return fail(MFM_E_STATE, "carry of %u samples, ring slots of %u", lp.carry_n, e->ring_slot);
        }
        hipLaunchKernelGGL(mfm_carry_kernel, dim3(1), dim3(256), 0, e->s_in, e->d_in[cur] + lp.carry_src, dst, lp.carry_n);
        HIP_TRY(hipGetLastError());
        /* this buffer is free once its kernel AND this copy are through (acquire_input waits for both) */
        HIP_TRY(hipEventRecord(e->tail_done[cur], e->s_in));
        e->tail_pending[cur] = true;
        e->head = dst;
        e->head_ev = e->tail_done[cur];
    } else if (LP_CARRY_COPY == lp.carrier) {
        const size_t ss = e->in_fmt[cur] != MFM_IN_CS16 ? 2 : 4;
        if (lp.two && e->in_free_wait[nxt]) {
            /* the launch that last read the next buffer may be on the other stream */
            HIP_TRY(hipStreamWaitEvent(S_after, e->in_free_wait[nxt], 0));
        }
        if (lp.two && e->tail_pending[nxt]) {
            /* ... and so may the carry copy OUT of that buffer, when a launch in between did not alternate:
             * a wait on a completed event costs nothing */
            HIP_TRY(hipStreamWaitEvent(S_after, e->tail_done[nxt], 0));
        }
        HIP_TRY(hipMemcpyAsync(e->d_in[nxt], reinterpret_cast<const uint8_t *>(e->d_in[cur]) + lp.carry_src * ss, lp.carry_n * ss,
                               hipMemcpyDeviceToDevice, S_after));
        if (lp.two) {
            /* this buffer is free once its kernel AND this copy are through (acquire_input waits for both) */
            HIP_TRY(hipEventRecord(e->tail_done[cur], S_after));
            e->tail_pending[cur] = true;
        }
    }
    return MFM_OK;
}

/* the outputs of the launch just queued on S: to the slot's host mirror on s_out, unless they stay on the device */
int queue_output(mfm_engine *e, const LaunchPlan &lp, OutSlot *slot, hipStream_t S)
{
    slot->first_output = e->outputs;
    slot->nr_outputs = lp.n_new;
    if (e->cfg.flags & MFM_F_DEVICE_ONLY) {
        /* nothing waits on slot->ready in device-only mode: consumers are ordered by the stream */
        return MFM_OK;
    }
    HIP_TRY(hipEventRecord(e->kernel_done, S));
    HIP_TRY(hipStreamWaitEvent(e->s_out, e->kernel_done, 0));
    const size_t row = (size_t)e->plan.out_stride * sizeof(int16_t), C = e->chans.size();
    HIP_TRY(hipMemcpy2DAsync(slot->h_pcm, row, slot->d_pcm, row, lp.n_new * sizeof(int16_t), C, hipMemcpyDeviceToHost, e->s_out));
    if (e->plan.any_iq) {
        HIP_TRY(hipMemcpy2DAsync(slot->h_iq, row * 2, slot->d_iq, row * 2, lp.n_new * sizeof(uint32_t), C, hipMemcpyDeviceToHost,
                                 e->s_out));
    }
    HIP_TRY(hipEventRecord(slot->ready, e->s_out));
    slot->state = OutSlot::INFLIGHT;
    return MFM_OK;
}

/*
 * One pass over d_in[cur_in] = [history tail | the blocks accepted since the last launch]: the kernel, the carry of the
 * unconsumed samples to where the next launch reads them, the copy of the outputs to the host mirror - queued as
 * launch_plan() (mfm_launch_plan.h) decides; every count and every choice of a stream is that plan's.  Caller holds e->mu
 * and has checked that an output slot is free.
 */
int launch_locked(mfm_engine *e)
{
    const LaunchPlan lp = launch_plan(launch_input(e));
    const int cur = e->cur_in, nxt = (cur + 1) % e->nbuf, fmt = e->in_fmt[cur];
    /* the stream of this launch, and of the one after it (the same one unless they alternate): what the next launch needs
     * from this buffer - the carry - is queued there */
    hipStream_t S = e->cs[e->si], S_after = lp.two ? e->cs[e->si ^ 1u] : S;
    if (e->head) {
        /* this buffer's [hist | tail] is in the ring: whoever reads it - the kernel or the copy below - comes behind its copy */
        HIP_TRY(hipStreamWaitEvent(S, e->head_ev, 0));
        if (LP_HEAD_COPY_BACK == lp.head) {
            hipLaunchKernelGGL(mfm_carry_kernel, dim3(1), dim3(256), 0, S, e->head, e->d_in[cur], lp.head_n);
            HIP_TRY(hipGetLastError());
            e->head = nullptr;
        }
    }
    if (lp.wait_next_reader && e->in_free_wait[nxt] && e->in_free_on[nxt] != S) {
        HIP_TRY(hipStreamWaitEvent(S, e->in_free_wait[nxt], 0));
    }

    OutSlot *slot = nullptr;
    int slot_idx = -1;
    if (lp.n_new) {
        slot_idx = (int)(e->submit_seq % e->nslots);
        slot = &e->slots[slot_idx];
        if (!(e->cfg.flags & MFM_F_DEVICE_ONLY) && slot->state != OutSlot::FREE) {
            return fail(MFM_E_BUSY, "all %d output slots hold unfetched blocks", e->nslots);
        }
    }
    if (e->wait_copy_stream) {
        HIP_TRY(hipEventRecord(e->in_ready, e->s_in));
        for (uint32_t i = 0; i < e->ncs; i++) {
            HIP_TRY(hipStreamWaitEvent(e->cs[i], e->in_ready, 0));
        }
        e->wait_copy_stream = false;
    }

    hipEvent_t timing_end = nullptr;
    if (lp.n_new) {
        int rc = queue_kernel(e, lp, e->plan.fmt[fmt], slot, S, &timing_end);
        if (rc != MFM_OK) {
            return rc;
        }
    }

    e->last_head = e->head;
    e->last_head_n = e->head ? lp.head_n : 0u;
    e->head = nullptr;
    int rc = queue_carry(e, lp, S_after);
    if (rc != MFM_OK) {
        return rc;
    }
    /* Every event record is a packet the command processor handles between two kernels (about 4 us each on
     * MI355X).  When the kernel carried the tail itself and its end is already stamped by the timing event, that
     * event also says "this input buffer is free". */
    if (LP_CARRY_KERNEL == lp.carrier && timing_end) {
        e->in_free_wait[cur] = timing_end;
    } else {
        HIP_TRY(hipEventRecord(e->in_free[cur], S));
        e->in_free_wait[cur] = e->in_free[cur];
    }
    e->in_free_on[cur] = S; /* (a later launch on the same stream is behind it anyway) */

    if (lp.n_new) {
        rc = queue_output(e, lp, slot, S);
        if (rc != MFM_OK) {
            return rc;
        }
        e->last_slot = slot_idx;
        e->s_last = S;
        e->submit_seq++;
        e->outputs += lp.n_new;
    }

    if (lp.two) {
        e->si ^= 1u;
    }
    e->pass++;
    e->last_launch_samples = lp.n_avail;
    e->last_launch_buf = cur;
    e->last_launch_fmt = fmt;
    e->last_launch_hist = e->hist;
    e->hist = lp.new_hist;
    e->tail = lp.new_tail;
    e->tail_fmt = fmt;
    e->in_fmt[cur] = MFM_IN_CS16;
    e->pend = 0;
    e->cur_in = nxt;
    return MFM_OK;
}

/* the buffer being filled holds blocks of another format than the one about to be accepted (a capture that changes its
 * sample format mid-stream; a cu8 block of odd length): what is there goes out as a launch of its own first */
int flush_for_format(mfm_engine *e, int fmt)
{
    if (0 == e->pend || e->in_fmt[e->cur_in] == fmt) {
        return MFM_OK;
    }
    std::lock_guard<std::mutex> guard(e->mu);
    return launch_locked(e);
}

} /* namespace */

extern "C" {

int mfm_engine_acquire_input(struct mfm_engine *e, void **d_dst, size_t *capacity_samples)
{
    if (!e || !d_dst) {
        return fail(MFM_E_INVAL, "NULL argument");
    }
    if (!e->committed) {
        return fail(MFM_E_STATE, "commit first");
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int rc = flush_for_format(e, MFM_IN_CS16);
    if (rc != MFM_OK) {
        return rc;
    }
    /* the kernel that last read this buffer (nbuf launches ago) must be done with it */
    if (e->in_free_wait[e->cur_in]) {
        HIP_TRY(hipEventSynchronize(e->in_free_wait[e->cur_in]));
        e->in_free_wait[e->cur_in] = nullptr; /* waited for: later blocks of this buffer need not ask again */
    }
    if (e->tail_pending[e->cur_in]) {
        HIP_TRY(hipEventSynchronize(e->tail_done[e->cur_in]));
        e->tail_pending[e->cur_in] = false;
    }
    if (0 == e->pend) {
        e->in_fmt[e->cur_in] = MFM_IN_CS16; /* what a device producer writes; mfm_engine_stage() says otherwise for raw bytes */
    }
    *d_dst = e->d_in[e->cur_in] + e->hist + e->tail + e->pend;
    if (capacity_samples) {
        *capacity_samples = std::min<size_t>(e->plan.cap_in - e->hist - e->tail - e->pend, e->cfg.max_block_samples);
    }
    return MFM_OK;
}

/* would the engine keep an 8-bit block of this format as bytes now?  (mfm_engine_internal.h) */
int mfm_engine_can_take_bytes(struct mfm_engine *e, int format, size_t nr_samples)
{
    /* not a cu8 block of odd length (file_if.c:146-150 widens its last sample differently), not behind a history or
     * behind accepted blocks of another format */
    if (!e || !e->committed || !e->plan.raw8_ok || !(format == MFM_IN_CS8 || format == MFM_IN_CU8 || format == MFM_IN_RTLSDR_U8) ||
        (format == MFM_IN_CU8 && (nr_samples & 1u))) {
        return 0;
    }
    const int bf = buffer_format(e);
    return bf == -1 || bf == format;
}

int mfm_engine_acquire_input_bytes(struct mfm_engine *e, int format, void **d_dst, size_t *capacity_samples)
{
    if (!e || !d_dst) {
        return fail(MFM_E_INVAL, "NULL argument");
    }
    if (!e->committed) {
        return fail(MFM_E_STATE, "commit first");
    }
    if (format != MFM_IN_CS8 && format != MFM_IN_CU8 && format != MFM_IN_RTLSDR_U8) {
        return fail(MFM_E_INVAL, "not an 8-bit sample format: %d", format);
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int rc = flush_for_format(e, format);
    if (rc != MFM_OK) {
        return rc;
    }
    if (!mfm_engine_can_take_bytes(e, format, 0)) {
        return fail(MFM_E_STATE, "this engine cannot read format %d as bytes now (kernel variant, or a history of another "
                                 "format): widen the block and use mfm_engine_acquire_input", format);
    }
    if (e->in_free_wait[e->cur_in]) {
        HIP_TRY(hipEventSynchronize(e->in_free_wait[e->cur_in]));
        e->in_free_wait[e->cur_in] = nullptr;
    }
    if (e->tail_pending[e->cur_in]) {
        HIP_TRY(hipEventSynchronize(e->tail_done[e->cur_in]));
        e->tail_pending[e->cur_in] = false;
    }
    e->in_fmt[e->cur_in] = format;
    *d_dst = reinterpret_cast<uint8_t *>(e->d_in[e->cur_in]) + ((size_t)e->hist + e->tail + e->pend) * 2;
    if (capacity_samples) {
        *capacity_samples = std::min<size_t>(e->plan.cap_in - e->hist - e->tail - e->pend, e->cfg.max_block_samples); /* the block limit is that of int16 blocks */
    }
    return MFM_OK;
}

/* mode: MFM_SUBMIT_AUTO - the engine decides whether the buffer is launched now (mfm_engine_config::coalesce_samples);
 * _DEFER / _LAUNCH - a device group has decided for all its shards (mfm_engine_internal.h) */
static int submit_impl(struct mfm_engine *e, size_t nr_samples, void *producer_stream, int wait_producer, int mode, bool run);

int mfm_engine_submit_mode(struct mfm_engine *e, size_t nr_samples, void *producer_stream, int wait_producer, int mode)
{
    return submit_impl(e, nr_samples, producer_stream, wait_producer, mode, false);
}

/* run: several blocks of at most max_block_samples each, staged next to each other, accepted as one (mfm_engine_push_pinned_run) */
static int submit_impl(struct mfm_engine *e, size_t nr_samples, void *producer_stream, int wait_producer, int mode, bool run)
{
    if (!e) {
        return fail(MFM_E_INVAL, "NULL engine");
    }
    if (!e->committed) {
        return fail(MFM_E_STATE, "commit first");
    }
    if (0 == nr_samples) {
        /* receiver_sample_buf_deliver() treats an empty buffer as a bug (receiver.c:84) */
        return fail(MFM_E_INVAL, "empty block");
    }
    if (nr_samples > (size_t)e->plan.cap_in - e->hist - e->tail - e->pend || (!run && nr_samples > e->cfg.max_block_samples)) {
        return fail(MFM_E_INVAL, "block of %zu samples exceeds max_block_samples %u", nr_samples,
                    e->cfg.max_block_samples);
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    std::lock_guard<std::mutex> guard(e->mu);

    const int cur = e->cur_in;
    const int fmt = e->in_fmt[cur];
    const bool raw8 = fmt != MFM_IN_CS16;
    if (raw8 && !mfm_engine_can_take_bytes(e, fmt, nr_samples)) {
        if (0 == e->pend) {
            e->in_fmt[cur] = MFM_IN_CS16;
        }
        return fail(MFM_E_INVAL, "a block of %zu samples of format %d cannot be read as bytes here (cu8 blocks must be of "
                                 "even length)", nr_samples, fmt);
    }

    SubmitPlan plan;
    plan_block(e, nr_samples, &plan, true);
    const bool launch = mode == MFM_SUBMIT_LAUNCH || (mode == MFM_SUBMIT_AUTO && (plan.must || (plan.want && plan.may)));
    if (launch && !plan.may) {
        return fail(MFM_E_BUSY, "all %d output slots hold unfetched blocks", e->nslots);
    }

    if (wait_producer && static_cast<hipStream_t>(producer_stream) == e->s_in && !launch) {
        e->wait_copy_stream = true; /* the launch that takes this block waits for the copy stream, once for all it gathered */
    } else if (wait_producer) {
        HIP_TRY(hipEventRecord(e->in_ready, static_cast<hipStream_t>(producer_stream)));
        for (uint32_t i = 0; i < e->ncs; i++) {
            HIP_TRY(hipStreamWaitEvent(e->cs[i], e->in_ready, 0)); /* the launch on one, the carry out of it on the other */
        }
        if (static_cast<hipStream_t>(producer_stream) == e->s_in) {
            e->wait_copy_stream = false; /* everything staged before is covered too */
        } else if (e->d_ring && e->ncs > 1u) {
            /* the early carry's copy runs on s_in and reads what this producer writes: behind it, and behind nothing else */
            HIP_TRY(hipStreamWaitEvent(e->s_in, e->in_ready, 0));
        }
    }

    if (!raw8 && 0 == e->pend && (e->hist + e->tail) && e->tail_fmt != MFM_IN_CS16) {
        /* the history at the front of this buffer is bytes, the block behind it int16: widen it where it stands (the
         * kernel that wrote it is ahead of this on the compute stream; the block's own samples start 4 * tail bytes in) */
        const uint32_t nh = e->hist + e->tail;
        hipStream_t Sn = e->cs[e->si]; /* the stream of this buffer's launch: the carry was queued there */
        HIP_TRY(hipMemcpyAsync(e->d_tailtmp, e->d_in[cur], (size_t)nh * 2, hipMemcpyDeviceToDevice, Sn));
        hipLaunchKernelGGL(mfm_unpack_kernel, dim3((nh / 8u + 256u) / 256u), dim3(256), 0, Sn, e->d_tailtmp,
                           e->d_in[cur], nh, e->tail_fmt, 0);
        HIP_TRY(hipGetLastError());
        e->tail_fmt = MFM_IN_CS16;
    }

    e->pend += (uint32_t)nr_samples;
    e->samples_in += nr_samples;
    e->submits++;
    return launch ? launch_locked(e) : MFM_OK;
}

int mfm_engine_submit(struct mfm_engine *e, size_t nr_samples, void *producer_stream, int wait_producer)
{
    return mfm_engine_submit_mode(e, nr_samples, producer_stream, wait_producer, MFM_SUBMIT_AUTO);
}

/* what accepting a block of nr_samples would mean for this engine (mfm_engine_internal.h) */
int mfm_engine_plan(struct mfm_engine *e, size_t nr_samples, int *must, int *may, int *want)
{
    if (!e || !e->committed) {
        return fail(MFM_E_STATE, "commit first");
    }
    if (hipSetDevice(e->cfg.device) != hipSuccess) {
        return fail(MFM_E_DEVICE, "hipSetDevice(%d) failed", e->cfg.device);
    }
    SubmitPlan p;
    plan_block(e, nr_samples, &p, false);
    *must = p.must ? 1 : 0;
    *may = p.may ? 1 : 0;
    *want = p.want ? 1 : 0;
    return MFM_OK;
}

int mfm_engine_format_conflict(struct mfm_engine *e, int fmt)
{
    return (e && e->committed && e->pend && e->in_fmt[e->cur_in] != fmt) ? 1 : 0;
}

int mfm_engine_flush(struct mfm_engine *e)
{
    if (!e || !e->committed) {
        return fail(MFM_E_STATE, "commit first");
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    /* pend is tested under the lock: two callers (a producer thread's idle flush and somebody else's sync) may get here at
     * once, and the second one must find nothing left to launch instead of launching an empty pass that rotates the
     * input buffers under the producer */
    std::lock_guard<std::mutex> guard(e->mu);
    if (0 == e->pend) {
        return MFM_OK;
    }
    return launch_locked(e);
}

/* would a block of nr_samples be accepted?  (refused before anything is staged, so a caller can drain and retry) */
static int check_output_room(struct mfm_engine *e, size_t nr_samples)
{
    SubmitPlan p;
    plan_block(e, nr_samples, &p, false);
    if (p.must && !p.may) {
        return fail(MFM_E_BUSY, "all %d output slots hold unfetched blocks", e->nslots);
    }
    return MFM_OK;
}

/*
 * Host -> device staging of one block WITHOUT submitting it (mfm_engine_internal.h): the samples (int16 pairs, or
 * 8-bit pairs widened on the device exactly as the reference's front ends widen them on the host) are placed where
 * the next submit() expects them, by work queued on the engine's copy stream.  *d_dst is that device address - what a
 * device group broadcasts to its other members before every member submits.
 */
int mfm_engine_stage(struct mfm_engine *e, const void *data, size_t nr_samples, int format, int flags, void **d_dst)
{
    const int allow_raw = flags & MFM_STAGE_ALLOW_RAW;
    const bool pinned = (flags & MFM_STAGE_PINNED) != 0; /* the caller's memory is page-locked: the copy engine reads it directly */
    if (!e || !data) {
        return fail(MFM_E_INVAL, "NULL argument");
    }
    if (format != MFM_IN_CS16 && format != MFM_IN_CS8 && format != MFM_IN_CU8 && format != MFM_IN_RTLSDR_U8) {
        return fail(MFM_E_INVAL, "unknown sample format %d", format);
    }
    if (!e->committed) {
        return fail(MFM_E_STATE, "commit first");
    }
    if (0 == nr_samples || nr_samples > e->cfg.max_block_samples) {
        return fail(MFM_E_INVAL, "block of %zu samples (max %u)", nr_samples, e->cfg.max_block_samples);
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    /* the matrix kernel reads the bytes themselves (mfm_kernel_v3.hip, IN8): half the HBM bytes, half the matrix
     * instructions, no widening pass.  Everything else goes the int16 way. */
    const bool raw = allow_raw && mfm_engine_can_take_bytes(e, format, nr_samples);
    int rc = flush_for_format(e, raw ? format : MFM_IN_CS16);
    if (rc != MFM_OK) {
        return rc;
    }
    rc = check_output_room(e, nr_samples);
    if (rc != MFM_OK) {
        return rc;
    }
    void *dst = nullptr;
    size_t cap = 0;
    rc = raw ? mfm_engine_acquire_input_bytes(e, format, &dst, &cap) : mfm_engine_acquire_input(e, &dst, &cap);
    if (rc != MFM_OK) {
        return rc;
    }
    if (cap < nr_samples) {
        return fail(MFM_E_INVAL, "the input buffer has room for %zu samples, the block has %zu", cap, nr_samples);
    }
    const int cur = e->cur_in;
    if (!pinned && !e->h_in[cur]) {
        HIP_TRY(hipHostMalloc(&e->h_in[cur], (size_t)e->plan.cap_in * 4, hipHostMallocDefault));
    }
    /* acquire_input() waited for the kernel that consumed the previous contents of this buffer, so the copies out of
     * h_in[cur] that fed it are done; blocks accepted since then sit in front of this one, as they do on the device */
    uint8_t *h = pinned ? const_cast<uint8_t *>(static_cast<const uint8_t *>(data))
                        : reinterpret_cast<uint8_t *>(e->h_in[cur]) + (size_t)e->pend * 4;
    if (raw) {
        if (!pinned) {
            memcpy(h, data, nr_samples * 2);
        }
        HIP_TRY(hipMemcpyAsync(dst, h, nr_samples * 2, hipMemcpyHostToDevice, e->s_in));
    } else if (format == MFM_IN_CS16) {
        if (!pinned) {
            memcpy(h, data, nr_samples * 4);
        }
        HIP_TRY(hipMemcpyAsync(dst, h, nr_samples * 4, hipMemcpyHostToDevice, e->s_in));
    } else {
        if (!e->d_raw[cur]) {
            HIP_TRY(hipMalloc(&e->d_raw[cur], (size_t)e->plan.cap_in * 2 + 64));
        }
        /* the unpack kernels of the previous use of d_raw[cur] ran before the kernel acquire_input() waited for */
        uint16_t *draw = e->d_raw[cur] + ((e->pend + 7u) & ~7u); /* the unpack kernel reads 16-byte groups */
        if (!pinned) {
            memcpy(h, data, nr_samples * 2);
        }
        HIP_TRY(hipMemcpyAsync(draw, h, nr_samples * 2, hipMemcpyHostToDevice, e->s_in));
        uint32_t blocks = (uint32_t)((nr_samples / 8 + 255) / 256);
        blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
        hipLaunchKernelGGL(mfm_unpack_kernel, dim3(blocks), dim3(256), 0, e->s_in, draw,
                           static_cast<uint32_t *>(dst), (uint32_t)nr_samples, format, 1);
        HIP_TRY(hipGetLastError());
    }
    if (pinned) {
        e->copy_seq++; /* this push's ticket (mfm_engine_copy_done / _wait) */
    }
    if (d_dst) {
        *d_dst = dst;
    }
    return MFM_OK;
}

uint64_t mfm_engine_copy_ticket(struct mfm_engine *e)
{
    return e ? e->copy_seq : 0;
}

/* is ticket through?  wait: block until it is.  Looks at the events that cover it; records one if none does. */
static int copy_ticket_state(struct mfm_engine *e, uint64_t ticket, bool wait)
{
    if (!e || !e->committed || ticket > e->copy_seq) {
        return fail(MFM_E_INVAL, "no such ticket");
    }
    if (ticket <= e->copy_done_seq) {
        return 1;
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    /* the oldest recorded event that covers the ticket answers soonest */
    int best = -1;
    for (int i = 0; i < (int)mfm_engine::kCopyRing; i++) {
        if (e->copy_ev_seq[i] >= ticket && (best < 0 || e->copy_ev_seq[i] < e->copy_ev_seq[best])) {
            best = i;
        }
    }
    if (best < 0) {
        /* none yet: one behind everything staged so far.  Its slot's previous event is the oldest one; if that is still
         * pending it covers only older tickets, and re-recording it loses nothing we are asked about. */
        best = (int)(e->copy_ev_next++ % mfm_engine::kCopyRing);
        if (!e->copy_ev[best]) {
            HIP_TRY(hipEventCreateWithFlags(&e->copy_ev[best], hipEventDisableTiming));
        }
        HIP_TRY(hipEventRecord(e->copy_ev[best], e->s_in));
        e->copy_ev_seq[best] = e->copy_seq;
    }
    if (wait) {
        HIP_TRY(hipEventSynchronize(e->copy_ev[best]));
    } else if (!event_done(e->copy_ev[best])) {
        return 0;
    }
    e->copy_done_seq = std::max(e->copy_done_seq, e->copy_ev_seq[best]);
    return 1;
}

int mfm_engine_copy_done(struct mfm_engine *e, uint64_t ticket)
{
    return copy_ticket_state(e, ticket, false);
}

int mfm_engine_copy_wait(struct mfm_engine *e, uint64_t ticket)
{
    const int rc = copy_ticket_state(e, ticket, true);
    return rc < 0 ? rc : MFM_OK;
}

int mfm_engine_push_pinned(struct mfm_engine *e, const void *data, size_t nr_samples, int format, uint64_t *ticket)
{
    int rc = mfm_engine_stage(e, data, nr_samples, format, MFM_STAGE_ALLOW_RAW | MFM_STAGE_PINNED, nullptr);
    if (rc != MFM_OK) {
        return rc;
    }
    if (ticket) {
        *ticket = e->copy_seq;
    }
    return mfm_engine_submit(e, nr_samples, e->s_in, 1);
}

size_t mfm_engine_input_room(struct mfm_engine *e)
{
    if (!e || !e->committed) {
        return 0;
    }
    std::lock_guard<std::mutex> guard(e->mu);
    return (size_t)e->plan.cap_in - e->hist - e->tail - e->pend;
}

/*
 * A run of `count` page-locked buffers of nr_samples_each samples that lie stride_bytes apart (the receiver's pool hands its
 * frames out in address order, so buffers delivered one after the other are neighbours in the arena): ONE strided copy command
 * packs them into the input buffer, and they are accepted as one block.  A copy command per 512 KiB sample_buf runs at half the
 * link's rate, one per 16 KiB file_if buffer at a ninth (bench.py end_to_end.link).  *accepted = how many of the buffers were
 * taken - fewer than `count` when the buffer being filled has less room, 1 where a block has to be widened on the device.
 */
int mfm_engine_push_pinned_run(struct mfm_engine *e, const void *first, size_t stride_bytes, size_t nr_samples_each, size_t count,
                               int format, uint64_t *ticket, size_t *accepted)
{
    if (accepted) {
        *accepted = 0;
    }
    if (!e || !first || 0 == count || 0 == nr_samples_each) {
        return fail(MFM_E_INVAL, "NULL or empty run");
    }
    if (!e->committed) {
        return fail(MFM_E_STATE, "commit first");
    }
    const size_t bps = (format == MFM_IN_CS16) ? 4u : 2u;
    if (nr_samples_each > e->cfg.max_block_samples || stride_bytes < nr_samples_each * bps) {
        return fail(MFM_E_INVAL, "run of blocks of %zu samples, %zu bytes apart (max block %u)", nr_samples_each, stride_bytes,
                    e->cfg.max_block_samples);
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    const bool raw = format != MFM_IN_CS16 && mfm_engine_can_take_bytes(e, format, nr_samples_each);
    size_t k = count;
    if (format != MFM_IN_CS16 && !raw) {
        k = 1; /* widened on the device through a scratch buffer: one block at a time */
    }
    if (k > 1) {
        /* what is there of another format goes out first (then the room is that of an empty buffer) */
        const int rcf = flush_for_format(e, raw ? format : MFM_IN_CS16);
        if (rcf != MFM_OK) {
            return rcf;
        }
        const size_t room = mfm_engine_input_room(e);
        k = std::min(k, room / nr_samples_each);
        /* a run must not gather past the point where the engine would have launched: what is gathered plus the run stays
         * within coalesce_samples + one block */
        const size_t co = e->cfg.coalesce_samples;
        if (co) {
            const size_t pend = (size_t)mfm_engine_pending_samples(e);
            const size_t until = co > pend ? (co - pend + nr_samples_each - 1u) / nr_samples_each : 1u;
            k = std::min(k, std::max<size_t>(until, 1u));
            /* ... and not at all where ONE buffer pushed by itself would launch right away (the device has nothing to do, or a
             * quarter of the running launch has gathered: plan_block's `want`): the first buffer goes alone, as per-buffer pushes
             * would have sent it, and the run behind it gathers under that launch */
            SubmitPlan one;
            plan_block(e, nr_samples_each, &one, false);
            if (one.want || one.must) {
                k = 1;
            }
        } else {
            k = 1; /* no gathering: every buffer is a launch of its own */
        }
    }
    if (k <= 1) {
        const int rc = mfm_engine_push_pinned(e, first, nr_samples_each, format, ticket);
        if (rc == MFM_OK && accepted) {
            *accepted = 1;
        }
        return rc;
    }
    const size_t total = nr_samples_each * k;
    int rc = check_output_room(e, total);
    if (rc != MFM_OK) {
        return rc;
    }
    void *dst = nullptr;
    size_t cap = 0;
    rc = raw ? mfm_engine_acquire_input_bytes(e, format, &dst, &cap) : mfm_engine_acquire_input(e, &dst, &cap);
    if (rc != MFM_OK) {
        return rc;
    }
    HIP_TRY(hipMemcpy2DAsync(dst, nr_samples_each * bps, first, stride_bytes, nr_samples_each * bps, k, hipMemcpyHostToDevice, e->s_in));
    e->copy_seq++; /* one ticket for the run: its copy is one command */
    if (ticket) {
        *ticket = e->copy_seq;
    }
    rc = submit_impl(e, total, e->s_in, 1, MFM_SUBMIT_AUTO, true);
    if (rc == MFM_OK && accepted) {
        *accepted = k;
    }
    return rc;
}

/* The host <-> device link by itself (include/multifm_hip.h): what a host-fed figure is to be read against. */
int mfm_link_probe(int device, size_t piece_bytes, size_t total_bytes, double d2h_per_h2d, double *h2d_GBps, double *d2h_GBps)
{
    return mfm_link_probe_runs(device, piece_bytes, 0, 1, total_bytes, d2h_per_h2d, h2d_GBps, d2h_GBps);
}

int mfm_link_probe_runs(int device, size_t piece_bytes, size_t gap_bytes, size_t pieces_per_command, size_t total_bytes,
                        double d2h_per_h2d, double *h2d_GBps, double *d2h_GBps)
{
    if (0 == piece_bytes || total_bytes < piece_bytes || d2h_per_h2d < 0.0 || d2h_per_h2d > 4.0 || 0 == pieces_per_command) {
        return fail(MFM_E_INVAL, "piece / total bytes, or the D2H share");
    }
    HIP_TRY(hipSetDevice(device));
    /* one arena of page-locked memory cut into pieces (gap_bytes apart: a sample_buf's header sits between the data of two
     * frames), like the receiver's sample_buf pool (host/mfm_receiver.c) */
    const size_t stride = piece_bytes + gap_bytes;
    size_t pieces_in_arena = std::max<size_t>(std::min<size_t>(total_bytes, (size_t)64 << 20) / stride, pieces_per_command);
    pieces_in_arena = pieces_in_arena / pieces_per_command * pieces_per_command;
    const size_t arena = pieces_in_arena * stride;
    const size_t back_piece = (size_t)((double)piece_bytes * d2h_per_h2d) & ~(size_t)15;
    uint8_t *h_src = nullptr, *h_dst = nullptr, *d_in = nullptr, *d_out = nullptr;
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr, f0 = nullptr, f1 = nullptr;
    int rc = MFM_OK;
    auto body = [&]() -> int {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h_src), arena, hipHostMallocDefault));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_in), pieces_in_arena * piece_bytes));
        memset(h_src, 0x5a, arena);
        if (back_piece) {
            HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h_dst), back_piece * pieces_in_arena, hipHostMallocDefault));
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_out), back_piece * pieces_in_arena));
            HIP_TRY(hipMemset(d_out, 0, back_piece * pieces_in_arena));
        }
        HIP_TRY(hipStreamCreateWithFlags(&s_in, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&s_out, hipStreamNonBlocking));
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventCreate(&f0));
        HIP_TRY(hipEventCreate(&f1));
        const size_t n = total_bytes / piece_bytes;
        for (int pass = 0; pass < 2; pass++) { /* the first pass warms the mappings up */
            HIP_TRY(hipEventRecord(e0, s_in));
            HIP_TRY(hipEventRecord(f0, s_out));
            for (size_t i = 0; i + pieces_per_command <= n; i += pieces_per_command) {
                const size_t k = i % pieces_in_arena;
                if (1 == pieces_per_command) {
                    HIP_TRY(hipMemcpyAsync(d_in + k * piece_bytes, h_src + k * stride, piece_bytes, hipMemcpyHostToDevice, s_in));
                } else {
                    /* a run of frames that lie next to each other in the arena: ONE strided command, packed on the device */
                    HIP_TRY(hipMemcpy2DAsync(d_in + k * piece_bytes, piece_bytes, h_src + k * stride, stride, piece_bytes,
                                             pieces_per_command, hipMemcpyHostToDevice, s_in));
                }
                if (back_piece) {
                    HIP_TRY(hipMemcpyAsync(h_dst + k * back_piece, d_out + k * back_piece, back_piece * pieces_per_command,
                                           hipMemcpyDeviceToHost, s_out));
                }
            }
            HIP_TRY(hipEventRecord(e1, s_in));
            HIP_TRY(hipEventRecord(f1, s_out));
            HIP_TRY(hipStreamSynchronize(s_in));
            HIP_TRY(hipStreamSynchronize(s_out));
        }
        float ms_in = 0.0f, ms_out = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms_in, e0, e1));
        HIP_TRY(hipEventElapsedTime(&ms_out, f0, f1));
        const size_t done = n / pieces_per_command * pieces_per_command;
        if (h2d_GBps) {
            *h2d_GBps = (double)(done * piece_bytes) / ((double)ms_in * 1e6);
        }
        if (d2h_GBps) {
            *d2h_GBps = back_piece ? (double)(done * back_piece) / ((double)ms_out * 1e6) : 0.0;
        }
        return MFM_OK;
    };
    rc = body();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (f0) (void)hipEventDestroy(f0);
    if (f1) (void)hipEventDestroy(f1);
    if (s_in) (void)hipStreamDestroy(s_in);
    if (s_out) (void)hipStreamDestroy(s_out);
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    (void)hipHostFree(h_src);
    (void)hipHostFree(h_dst);
    return rc;
}

void *mfm_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (0 == bytes || hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

void mfm_host_free(void *p)
{
    if (p) {
        (void)hipHostFree(p);
    }
}

void *mfm_engine_copy_stream(struct mfm_engine *e)
{
    return (e && e->committed) ? e->s_in : nullptr;
}

int mfm_engine_pending_blocks(struct mfm_engine *e)
{
    if (!e || !e->committed) {
        return 0;
    }
    std::lock_guard<std::mutex> guard(e->mu);
    return (int)(e->submit_seq - e->fetch_seq);
}

int mfm_engine_pending_samples(struct mfm_engine *e)
{
    if (!e || !e->committed) {
        return 0;
    }
    std::lock_guard<std::mutex> guard(e->mu);
    return (int)e->pend;
}

int mfm_engine_push(struct mfm_engine *e, const int16_t *iq, size_t nr_samples)
{
    const int rc = mfm_engine_stage(e, iq, nr_samples, MFM_IN_CS16, 0, nullptr);
    return rc != MFM_OK ? rc : mfm_engine_submit(e, nr_samples, e->s_in, 1);
}

int mfm_engine_push_bytes(struct mfm_engine *e, const void *bytes, size_t nr_samples, int format)
{
    const int rc = mfm_engine_stage(e, bytes, nr_samples, format, MFM_STAGE_ALLOW_RAW, nullptr);
    return rc != MFM_OK ? rc : mfm_engine_submit(e, nr_samples, e->s_in, 1);
}

int mfm_engine_last_launch_input(struct mfm_engine *e, void **d_in, size_t *nr_samples, int *format)
{
    if (!e || !e->committed || e->last_launch_buf < 0) {
        return fail(MFM_E_STATE, "no launch yet");
    }
    if (e->last_head) {
        /* the launch read its first samples from the carry ring: they go where this call promises them, once the launch
         * (the only reader of the buffer's front, if it looked there at all) is through */
        HIP_TRY(hipSetDevice(e->cfg.device));
        HIP_TRY(hipStreamSynchronize(e->s_last));
        HIP_TRY(hipMemcpyAsync(e->d_in[e->last_launch_buf], e->last_head, (size_t)e->last_head_n * 4, hipMemcpyDeviceToDevice,
                               e->s_last));
        HIP_TRY(hipStreamSynchronize(e->s_last));
        e->last_head = nullptr;
    }
    if (d_in) {
        /* the first sample the launch had not consumed before (the second-generation kernel keeps a row in front of it) */
        *d_in = reinterpret_cast<uint8_t *>(e->d_in[e->last_launch_buf]) +
                (size_t)e->last_launch_hist * (e->last_launch_fmt == MFM_IN_CS16 ? 4 : 2);
    }
    if (nr_samples) {
        *nr_samples = e->last_launch_samples;
    }
    if (format) {
        *format = e->last_launch_fmt;
    }
    return MFM_OK;
}

int mfm_engine_replay(struct mfm_engine *e, size_t block_samples, size_t nr_blocks)
{
    for (size_t i = 0; i < nr_blocks; i++) {
        void *dst = nullptr;
        size_t cap = 0;
        int rc = mfm_engine_acquire_input(e, &dst, &cap);
        if (rc != MFM_OK) {
            return rc;
        }
        if (cap < block_samples) {
            return fail(MFM_E_INVAL, "replay: block of %zu samples, room for %zu", block_samples, cap);
        }
        rc = mfm_engine_submit(e, block_samples, nullptr, 0);
        if (rc != MFM_OK) {
            return rc;
        }
    }
    return MFM_OK;
}


int mfm_engine_fetch(struct mfm_engine *e, struct mfm_block *blk)
{
    if (!e || !blk) {
        return fail(MFM_E_INVAL, "NULL argument");
    }
    if (!e->committed || (e->cfg.flags & MFM_F_DEVICE_ONLY)) {
        return fail(MFM_E_STATE, "fetch needs a committed engine without MFM_F_DEVICE_ONLY");
    }
    OutSlot *sp = nullptr;
    {
        std::lock_guard<std::mutex> guard(e->mu);
        if (e->fetch_seq >= e->submit_seq) {
            return MFM_E_DONE;
        }
        sp = &e->slots[e->fetch_seq % e->nslots];
        if (sp->state == OutSlot::FETCHED) {
            return fail(MFM_E_STATE, "release the previous block first");
        }
    }
    OutSlot &s = *sp;
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipEventSynchronize(s.ready)); /* outside the lock: the producer keeps submitting meanwhile */
    std::lock_guard<std::mutex> guard(e->mu);
    s.state = OutSlot::FETCHED;
    blk->first_output = s.first_output;
    blk->nr_outputs = s.nr_outputs;
    blk->stride = e->plan.out_stride;
    blk->pcm = s.h_pcm;
    blk->iq = reinterpret_cast<const int16_t *>(s.h_iq);
    return MFM_OK;
}

int mfm_engine_release(struct mfm_engine *e)
{
    if (!e) {
        return fail(MFM_E_INVAL, "NULL engine");
    }
    std::lock_guard<std::mutex> guard(e->mu);
    if (!e->committed || e->fetch_seq >= e->submit_seq) {
        return fail(MFM_E_STATE, "nothing fetched");
    }
    OutSlot &s = e->slots[e->fetch_seq % e->nslots];
    if (s.state != OutSlot::FETCHED) {
        return fail(MFM_E_STATE, "nothing fetched");
    }
    s.state = OutSlot::FREE;
    e->fetch_seq++;
    return MFM_OK;
}

int mfm_engine_last_output_device(struct mfm_engine *e, void **d_pcm, size_t *stride, size_t *nr_outputs,
                                  void **d_iq)
{
    if (!e || !e->committed || e->last_slot < 0) {
        return fail(MFM_E_STATE, "no output yet");
    }
    const OutSlot &s = e->slots[e->last_slot];
    if (d_pcm) {
        *d_pcm = s.d_pcm;
    }
    if (stride) {
        *stride = e->plan.out_stride;
    }
    if (nr_outputs) {
        *nr_outputs = s.nr_outputs;
    }
    if (d_iq) {
        *d_iq = s.d_iq;
    }
    return MFM_OK;
}

int mfm_engine_sync(struct mfm_engine *e)
{
    if (!e || !e->committed) {
        return fail(MFM_E_STATE, "commit first");
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    /* what has been accepted and not launched goes out first (MFM_E_BUSY: the caller fetches / releases and syncs again) */
    const int rc = mfm_engine_flush(e);
    if (rc != MFM_OK) {
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(e->s_in));
    HIP_TRY(hipStreamSynchronize(e->s_compute));
    if (e->cs[1] != e->s_compute) {
        HIP_TRY(hipStreamSynchronize(e->cs[1]));
    }
    if (e->s_out) {
        HIP_TRY(hipStreamSynchronize(e->s_out));
    }
    return MFM_OK;
}

int mfm_engine_reset(struct mfm_engine *e)
{
    if (!e || !e->committed) {
        return fail(MFM_E_STATE, "commit first");
    }
    /* pending blocks are dropped, accepted-but-unlaunched samples with them */
    e->pend = 0;
    int rc = mfm_engine_sync(e);
    if (rc != MFM_OK) {
        return rc;
    }
    rc = write_state_fresh(e);
    if (rc != MFM_OK) {
        return rc;
    }
    for (int i = 0; i < e->nslots; i++) {
        e->slots[i].state = OutSlot::FREE;
    }
    e->fetch_seq = e->submit_seq = 0;
    e->last_slot = -1;
    e->tail = 0;
    e->hist = 0;
    e->tail_fmt = MFM_IN_CS16;
    e->in_fmt[0] = e->in_fmt[1] = e->in_fmt[2] = MFM_IN_CS16;
    e->cur_in = 0;
    e->pass = 0; /* (buffer pass % nbuf again; the carry ring's slots are all free: everything has ended) */
    e->head = e->last_head = nullptr;
    e->last_head_n = 0;
    for (int i = 0; i < kMaxInBufs; i++) {
        e->in_free_wait[i] = nullptr;
        e->tail_pending[i] = false;
    }
    e->wait_copy_stream = false;
    e->last_launch_samples = 0;
    e->last_launch_buf = -1;
    e->outputs = 0;
    e->samples_in = 0;
    return MFM_OK;
}

int mfm_engine_seek(struct mfm_engine *e, uint64_t outputs_before)
{
    int rc = mfm_engine_reset(e);
    if (rc != MFM_OK) {
        return rc;
    }
    /* the rotators stand where outputs_before steps of the recurrence leave them (filter/direct_fir.c:166-167); the
     * second-generation kernel folds the count itself, the others read the folded table position from the carried state */
    std::vector<mfm_chan_state> st(e->plan.ngroups * MFM_CG);
    for (size_t c = 0; c < st.size(); c++) {
        st[c].carry_q = 0;
        st[c].kb = 0;
        if (c < e->chans.size()) {
            const Channel &ch = e->chans[c];
            st[c].kb = outputs_before < ch.mu ? (uint32_t)outputs_before : ch.mu + (uint32_t)((outputs_before - ch.mu) % ch.lam);
        }
    }
    for (int i = 0; i < 2; i++) {
        HIP_TRY(hipMemcpy(e->d_state[i], st.data(), st.size() * sizeof(mfm_chan_state), hipMemcpyHostToDevice));
    }
    e->outputs = outputs_before;
    return MFM_OK;
}

int mfm_engine_get_stats(struct mfm_engine *e, struct mfm_stats *st)
{
    if (!e || !st) {
        return fail(MFM_E_INVAL, "NULL argument");
    }
    memset(st, 0, sizeof(*st));
    if (e->committed && (e->cfg.flags & MFM_F_TIMING)) {
        HIP_TRY(hipSetDevice(e->cfg.device));
        std::lock_guard<std::mutex> guard(e->mu); /* (the producer appends to what is folded here) */
        int rc = fold_timing(e, true);
        if (rc != MFM_OK) {
            return rc;
        }
    }
    st->samples_in = e->samples_in;
    st->outputs = e->outputs;
    st->launches = e->launches;
    st->kernel_ms = e->kernel_ms;
    st->timed_launches = e->launch_ms_n;
    plan_form_stats(e->plan, st);
    st->submits = e->submits;
    st->nr_channels = (uint32_t)e->chans.size();
    st->nr_taps = e->nr_taps;
    {
        std::lock_guard<std::mutex> guard(e->mu);
        st->pending_blocks = (uint32_t)(e->submit_seq - e->fetch_seq);
        st->pending_samples = e->pend; /* written under the lock by submit / launch */
        st->launches_8bit = e->launches_8bit;
        st->overlapped_launches = e->overlapped;
        st->pinned = e->pinned ? 1u : 0u;
    }
    st->grid_last = e->grid_last;
    st->tail_samples = e->tail;
    st->rot_table_entries = e->rot_entries;
    return MFM_OK;
}

size_t mfm_engine_get_launch_ms(struct mfm_engine *e, float *dst, size_t cap)
{
    if (!e || !e->committed || !(e->cfg.flags & MFM_F_TIMING)) {
        return 0;
    }
    std::lock_guard<std::mutex> guard(e->mu);
    if (hipSetDevice(e->cfg.device) != hipSuccess || fold_timing(e, true) != MFM_OK) {
        return 0;
    }
    const size_t have = (size_t)std::min<uint64_t>(e->launch_ms_n, kLaunchRing);
    const size_t n = std::min(have, cap);
    for (size_t i = 0; i < n && dst; i++) {
        dst[i] = e->launch_ms[(e->launch_ms_n - n + i) % kLaunchRing];
    }
    return n;
}

size_t mfm_engine_get_launch_cycles(struct mfm_engine *e, uint64_t *shader_ticks, uint64_t *ref_ticks, size_t cap)
{
    if (!e || !e->committed || !e->d_cyc) {
        return 0;
    }
    /* Only what HAS been launched is waited for: this is a read-only call (also on the engines of a device group, from whatever
     * thread looks at the figures) - a flush from here would launch one shard of a gathering group by itself and take the
     * shards out of step. */
    if (hipSetDevice(e->cfg.device) != hipSuccess || hipStreamSynchronize(e->s_compute) != hipSuccess ||
        (e->cs[1] != e->s_compute && hipStreamSynchronize(e->cs[1]) != hipSuccess)) {
        return 0;
    }
    std::vector<unsigned long long> ring(kCycleRing * 2);
    if (hipMemcpy(ring.data(), e->d_cyc, ring.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) {
        return 0;
    }
    /* (a launch clears the slot half a ring ahead of its own: the newer half of the ring is what can be read) */
    const uint64_t have = std::min<uint64_t>(e->launches, kCycleRing / 2u);
    const size_t n = (size_t)std::min<uint64_t>(have, cap);
    for (size_t i = 0; i < n; i++) {
        const uint64_t seq = e->launches - n + i; /* 0-based index of the launch */
        const uint64_t tag = ((seq + 1u) & 0xffffffu) << 40, mask = (1ull << 40) - 1ull;
        const unsigned long long a = ring[2 * (seq % kCycleRing)], b = ring[2 * (seq % kCycleRing) + 1];
        if (shader_ticks) {
            shader_ticks[i] = (a & ~mask) == tag ? (a & mask) : 0u; /* 0: the launch left no stamp (no work, or not this kernel) */
        }
        if (ref_ticks) {
            ref_ticks[i] = (b & ~mask) == tag ? (b & mask) : 0u;
        }
    }
    return n;
}

/* The stream is handed out (or a device group takes the engine): one compute stream from here on, unless MFM_F_OVERLAP asked
 * for two.  s_compute waits for the other stream's last launch and becomes the stream of every later one; a head that is
 * still in the carry ring goes to its buffer's front with the next launch (launch_locked). */
int mfm_engine_pin(struct mfm_engine *e)
{
    if (!e || !e->committed) {
        return fail(MFM_E_STATE, "commit first");
    }
    std::lock_guard<std::mutex> guard(e->mu);
    if (e->pinned || (e->cfg.flags & MFM_F_OVERLAP)) {
        return MFM_OK;
    }
    e->pinned = true;
    if (e->ncs > 1u) {
        HIP_TRY(hipSetDevice(e->cfg.device));
        HIP_TRY(hipEventRecord(e->kernel_done, e->cs[1])); /* (device-only engines have no other use for this event) */
        HIP_TRY(hipStreamWaitEvent(e->cs[0], e->kernel_done, 0));
        e->ncs = 1;
        e->si = 0;
        e->s_last = e->cs[0];
    }
    return MFM_OK;
}

void *mfm_engine_stream(struct mfm_engine *e)
{
    if (!e || !e->committed) {
        return nullptr;
    }
    if (mfm_engine_pin(e) != MFM_OK) {
        return nullptr;
    }
    return e->s_last;
}

/* ---- host twins (see include/multifm_hip.h) ---- */

static float g_atan_tbl[257];
static float2 g_atan_lut[256];
static bool g_atan_ok = false;
static void atan_tbl_once(void);

int mfm_devtest_rcp_table(int device, uint64_t *hash, uint64_t counts[4], uint64_t *sweep_bad, uint64_t *sweep_tried)
{
    if (!hash || !counts) {
        return fail(MFM_E_INVAL, "bad argument");
    }
    uint64_t t[5];
    int rc = rcp_table_read(device, t);
    if (rc != MFM_OK) {
        return rc;
    }
    *hash = t[0];
    counts[0] = t[1];
    counts[1] = t[2];
    counts[2] = t[3];
    counts[3] = t[4];
    if (sweep_bad && sweep_tried) {
        rc = div_sweep(device, sweep_bad, sweep_tried);
    }
    return rc;
}

/* the discriminator as the kernels of variant 0 / 1 / 2 compute it, on the device, for caller-supplied products */
int mfm_devtest_discriminate(int variant, const int32_t *s_re, const int32_t *s_im, size_t n, int16_t *pcm_out, int device)
{
    if (!s_re || !s_im || !pcm_out || variant < 0 || variant > 2 || n > (1u << 28)) {
        return fail(MFM_E_INVAL, "bad argument");
    }
    if (0 == n) {
        return MFM_OK;
    }
    atan_tbl_once();
    HIP_TRY(hipSetDevice(device));
    const size_t np = (n + 3u) & ~(size_t)3u;
    int *d_re = nullptr, *d_im = nullptr, *d_out = nullptr;
    float2 *d_lut = nullptr;
    int rc = MFM_OK;
    std::vector<int32_t> out(np);
    do {
        if (hipMalloc(&d_re, np * 4) != hipSuccess || hipMalloc(&d_im, np * 4) != hipSuccess || hipMalloc(&d_out, np * 4) != hipSuccess ||
            hipMalloc(&d_lut, sizeof(g_atan_lut)) != hipSuccess) {
            rc = fail(MFM_E_NOMEM, "device allocation failed");
            break;
        }
        if (hipMemset(d_re, 0, np * 4) != hipSuccess || hipMemset(d_im, 0, np * 4) != hipSuccess ||
            hipMemcpy(d_re, s_re, n * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_im, s_im, n * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_lut, g_atan_lut, sizeof(g_atan_lut), hipMemcpyHostToDevice) != hipSuccess) {
            rc = fail(MFM_E_DEVICE, "copy to the device failed");
            break;
        }
        const hipError_t err = variant == 2   ? mfm_disc_test_v3(d_re, d_im, d_out, (uint32_t)np, d_lut, nullptr)
                               : variant == 1 ? mfm_disc_test_mfma(d_re, d_im, d_out, (uint32_t)np, d_lut, nullptr)
                                              : mfm_disc_test_dot2(d_re, d_im, d_out, (uint32_t)np, d_lut, nullptr);
        if (err != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(out.data(), d_out, np * 4, hipMemcpyDeviceToHost) != hipSuccess) {
            rc = fail(MFM_E_DEVICE, "discriminator test kernel failed: %s", hipGetErrorString(err));
            break;
        }
        for (size_t i = 0; i < n; i++) {
            pcm_out[i] = (int16_t)out[i];
        }
    } while (0);
    (void)hipFree(d_re);
    (void)hipFree(d_im);
    (void)hipFree(d_out);
    (void)hipFree(d_lut);
    return rc;
}

static void atan_tbl_build(void)
{
    /* multifm/fast_atan2f.c:14-81: the reference's literals are atan(i/255) printed with seven
     * significant digits; entry 256 repeats entry 255 (the index+1 read at :131). */
    for (int i = 0; i < 257; i++) {
        char txt[32];
        const int k = i < 255 ? i : 255;
        snprintf(txt, sizeof(txt), "%.6e", atan((double)k / 255.0));
        g_atan_tbl[i] = strtof(txt, nullptr);
    }
    for (int i = 0; i < 256; i++) {
        g_atan_lut[i] = make_float2(g_atan_tbl[i], g_atan_tbl[i + 1] - g_atan_tbl[i]);
    }
    /* FNV-1a over the 257 bit patterns; the constant was checked against values read back through
     * the reference's own fast_atan2f() (tests/test_oracle_atan2.py). A libm that rounds atan
     * differently at the 7th digit would trip this instead of silently changing PCM. */
    uint64_t h = 1469598103934665603ull;
    for (int i = 0; i < 257; i++) {
        uint32_t b;
        memcpy(&b, &g_atan_tbl[i], 4);
        for (int k = 0; k < 4; k++) {
            h ^= (b >> (8 * k)) & 0xffu;
            h *= 1099511628211ull;
        }
    }
    g_atan_ok = (h == MFM_ATAN_TABLE_FNV1A);
}

static void atan_tbl_once(void)
{
    static std::once_flag once;
    std::call_once(once, atan_tbl_build);
}

int mfm_hosttwin_atan_table_ok(void)
{
    atan_tbl_once();
    return g_atan_ok ? 1 : 0;
}

void mfm_hosttwin_atan_table(float tbl[257])
{
    atan_tbl_once();
    memcpy(tbl, g_atan_tbl, sizeof(g_atan_tbl));
}

int32_t mfm_hosttwin_discriminate(int32_t s_re, int32_t s_im)
{
    atan_tbl_once();
    return mfm_discriminate(s_re, s_im, g_atan_lut);
}

void mfm_hosttwin_discriminate_batch(const int32_t *s_re, const int32_t *s_im, size_t n, int16_t *out)
{
    atan_tbl_once();
    for (size_t i = 0; i < n; i++) {
        out[i] = (int16_t)mfm_discriminate(s_re[i], s_im[i], g_atan_lut);
    }
}

int mfm_hosttwin_kernel_form(struct mfm_engine *e, struct mfm_stats *st)
{
    if (!e || !st) {
        return fail(MFM_E_INVAL, "NULL argument");
    }
    if (e->committed) {
        return fail(MFM_E_STATE, "already committed: mfm_engine_get_stats() reports the form");
    }
    KernelPlan p;
    const int rc = plan_channel_kernel(e->cfg, e->chans, e->nr_taps, p);
    if (rc != MFM_OK) {
        return rc;
    }
    memset(st, 0, sizeof(*st));
    plan_form_stats(p, st);
    return MFM_OK;
}

int16_t mfm_hosttwin_r14(int32_t a)
{
    return (int16_t)mfm_r14_wide(a);
}

void mfm_hosttwin_pcm_range(uint32_t first_bits, uint32_t count, int16_t *out)
{
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t b = first_bits + i;
        float m;
        memcpy(&m, &b, 4);
        out[i] = (int16_t)mfm_mag_to_pcm(m);
    }
}

} /* extern "C" */
