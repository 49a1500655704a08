/*
 * mfm_level_adaptive.hip - the finish kernel of the level stage's adaptive squelch (include/multifm_hip.h:
 * mfm_level_set_adaptive), an object of its own so that mfm_level.o keeps the three kernels it had.  mfm_level.hip holds the
 * setting and the buffers and queues this kernel in the place of lv_finish_kernel; the arithmetic is mfm_level.h's, which the
 * host twin (mfm_hosttwin_level_adaptive) runs too, the window sums are mfm_level_kernels.h's, which lv_finish_kernel runs too.
 *
 * One wave per channel.  The channel's sequence of KEYS (mfm_level_floor_key: one sliding minimum serves both senses) is
 * [the H = M - 1 windows in front of the call, from the device history | the call's windows], and the floor of the call's
 * window j is the minimum of entries j .. j + H of it.  The sequence goes through LDS in strips of at most LV_STRIP windows
 * (H + LV_STRIP <= 2047 entries, twice: 32 752 bytes at most):
 *
 *   fill      rounds of 64 windows: the window sums as in lv_finish_kernel, the records without .open, the keys into `raw`
 *   doubling  work[i] = min(raw[i .. i + 2^p - 1]), 2^p the largest power of two <= M, in p passes over the strip (pass t takes
 *             the minimum with the entry 2^t further on; in place, chunks of 64 ascending, so an entry is read before the pass
 *             overwrites it): log2(M) steps per window whatever M is
 *   squelch   rounds of 64 windows: floor = min(work[j], work[j + M - 2^p]) (two overlapping spans of 2^p cover M entries),
 *             both predicates per lane, balloted into two 64-bit masks; the sequential part walks the masks with scalar code
 *             (a shift, two bit tests and the state machine per step: no lane reads, no 64-bit compares), and lane j keeps step j
 *
 * Windows in front of the first one after create / seek have the identity as key; how many of the history's entries exist
 * follows from the stream position (A.done), so a seek leaves the history buffer as it is.  No float, no atomics, no scratch.
 */
#include <hip/hip_runtime.h>

#include "../../include/multifm_hip.h"
#include "mfm_level.h"
#include "mfm_level_kernels.h"

namespace {

using namespace mfm_lv;

__global__ __launch_bounds__(64) void lv_adaptive_finish_kernel(const LvFinish L, const LvAdaptive A)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t lv_strip[];
    const uint32_t lane = threadIdx.x;
    const uint32_t c = blockIdx.x;
    /* the channel's state in VECTOR registers (an offset the compiler cannot see through makes the load a vector load): the
     * arguments fill the scalar file, and all but open / bad are needed in two places only.  What tools/kernel_regs.py reads off
     * the object (ROCm 7.2 hipcc, -O3): with the plain L.st[c], a scalar load that keeps the eight dwords live in scalar registers
     * throughout, vgpr 49, sgpr 106 (the whole file) and 2 scalar registers spilled; with this, vgpr 52, sgpr 104, no spill.  If a
     * compiler leaves the plain form without a spill, these three lines can go (tests/test_level_adaptive.py reads the counts). */
    uint32_t zero = 0;
    asm volatile("" : "+v"(zero));
    const LvChan s = L.st[c + zero];
    const LvPart *pc = L.parts + (size_t)c * L.parts_stride;
    mfm_level_record *rc = L.rec + (size_t)c * L.rec_stride;
    uint64_t *fl = A.floor + (size_t)c * A.floor_stride;
    uint64_t *hc = A.hist + (size_t)c * A.hist_stride;
    const uint32_t H = A.M - 1u;
    const uint32_t cap = H + (L.nwin < LV_STRIP ? L.nwin : LV_STRIP); /* entries of a strip at most: the launcher's LDS size */
    uint64_t *raw = lv_strip, *work = lv_strip + cap;
    const uint32_t span = 1u << (31 - __clz((int)A.M));               /* largest power of two <= M */
    const uint32_t have = A.done < H ? (uint32_t)A.done : H;          /* history entries that exist: the last `have` */
    const uint32_t below = L.Q.below;
    /* the same in every lane: in scalar registers, so that the walk below is scalar code */
    uint32_t open = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.open), bad = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.bad);
    uint32_t n = 0;
    for (uint32_t w0 = 0; w0 < L.nwin; w0 += LV_STRIP) {
        n = L.nwin - w0 < LV_STRIP ? L.nwin - w0 : LV_STRIP;
        const uint32_t len = H + n;
        /* the H keys in front of the strip: the device history, or the end of the strip before (which was a full one) */
        for (uint32_t i = lane; i < H; i += 64) {
            raw[i] = w0 ? raw[LV_STRIP + i] : (i < H - have ? ~0ull : hc[i]);
        }
        __syncthreads(); /* (a block is one wave: the barriers order its LDS traffic, nobody waits for anybody) */
        for (uint32_t m0 = 0; m0 < n; m0 += 64) {
            const uint32_t cnt = n - m0 < 64u ? n - m0 : 64u;
            uint64_t e, d;
            uint32_t p;
            lv_round_sums(L, s, pc, lane, w0 + m0, cnt, e, d, p);
            if (lane < cnt) {
                const uint32_t m = w0 + m0 + lane;
                rc[m].energy = e;
                rc[m].diff_energy = d;
                rc[m].window = L.k0 + m;
                rc[m].peak = p;
                rc[m].channel = c;
                rc[m].reserved = 0;
                raw[H + m0 + lane] = mfm_level_floor_key(below, L.Q.use_diff ? d : e);
            }
        }
        __syncthreads();
        for (uint32_t i = lane; i < len; i += 64) {
            const uint64_t a = raw[i];
            const uint64_t b = span > 1u && i + 1u < len ? raw[i + 1u] : a;
            work[i] = b < a ? b : a;
        }
        __syncthreads();
        for (uint32_t step = 2; step < span; step <<= 1) {
            for (uint32_t i0 = 0; i0 < len; i0 += 64) {
                const uint32_t i = i0 + lane;
                uint64_t a = 0, b = 0;
                if (i < len) {
                    a = work[i];
                    b = i + step < len ? work[i + step] : a;
                }
                __syncthreads(); /* every read of the chunk before any of its writes */
                if (i < len) {
                    work[i] = b < a ? b : a;
                }
            }
            __syncthreads();
        }
        for (uint32_t m0 = 0; m0 < n; m0 += 64) {
            const uint32_t cnt = n - m0 < 64u ? n - m0 : 64u;
            const uint32_t j = m0 + lane;
            const bool act = lane < cnt;
            bool o = false, b = false;
            uint64_t floor = 0;
            if (act) {
                const uint64_t key = raw[H + j];
                const uint64_t f0 = work[j], f1 = work[j + A.M - span];
                const uint64_t fkey = f1 < f0 ? f1 : f0;
                floor = mfm_level_floor_key(below, fkey);
                const bool warm = A.done + w0 + j < (uint64_t)A.warmup;
                mfm_level_adaptive_predicates(below, mfm_level_floor_key(below, key), floor, A.open_q8, A.close_q8, L.Q.open_thr, L.Q.close_thr,
                                              warm, o, b);
            }
            const uint64_t on_open_side = __ballot(o), is_bad = __ballot(b);
            uint64_t after = 0; /* bit j: the squelch after step j */
            for (uint32_t k = 0; k < cnt; k++) {
                mfm_level_squelch_step_bits(open, bad, L.Q.hang, (on_open_side >> k) & 1ull, (is_bad >> k) & 1ull);
                after |= (uint64_t)open << k;
            }
            if (act) {
                rc[w0 + j].open = (uint32_t)(after >> lane) & 1u;
                fl[w0 + j] = floor;
            }
        }
        __syncthreads(); /* the next strip's front is read from this one's end */
    }
    if (L.nwin) { /* the history behind the call: the last H keys of the last strip */
        for (uint32_t i = lane; i < H; i += 64) {
            hc[i] = raw[n + i];
        }
    }
    lv_leave(L, s, pc, lane, c, open, bad);
}

} /* namespace */

extern "C" __attribute__((visibility("hidden"))) int mfm_internal_level_adaptive_launch(const mfm_lv::LvFinish *finish,
                                                                                         const mfm_lv::LvAdaptive *adaptive,
                                                                                         uint32_t nr_channels, hipStream_t s)
{
    const LvFinish &L = *finish;
    const LvAdaptive &A = *adaptive;
    if (0 == A.M || A.M > LV_STRIP) {
        return MFM_E_INVAL; /* the strip is sized for M - 1 <= LV_STRIP - 1 entries in front */
    }
    const uint32_t cap = A.M - 1u + (L.nwin < LV_STRIP ? L.nwin : LV_STRIP);
    hipLaunchKernelGGL(lv_adaptive_finish_kernel, dim3(nr_channels), dim3(64), (size_t)cap * 16u, s, L, A);
    return hipGetLastError() == hipSuccess ? MFM_OK : MFM_E_DEVICE;
}
