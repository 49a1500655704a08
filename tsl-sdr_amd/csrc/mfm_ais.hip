/*
 * mfm_ais.hip - the AIS stage behind the PCM resampler, batched over all channels on the GPU: slicer, preamble
 * detector, NRZI / HDLC bit recovery and the FCS check (ais/ais_demod.c:19-36,114-258).  See
 * include/multifm_hip.h for the boundary and the event format.
 *
 * The reference walks one 48 kHz sample at a time through a two-state machine.  What is data parallel in it, and
 * how it is laid out here (per channel, all in HBM, 1 bit per sample):
 *
 *   bits    b[s] = (pcm[s] > 0), the slicer (ais_demod.c:126).
 *   match   M[t] = "at least three of the five preamble registers match after sample t" (:135-145).  With the
 *           detector's NRZI bit n[s] = !(b[s] ^ b[s-5]), the register last updated at t holds R(t), bit k =
 *           n[t - 5k], and q[t] = popcount(R(t) ^ 0x5555557e) <= 2; M[t] = q[t] + ... + q[t-4] >= 3.  Computed
 *           32 samples at a time, bit-sliced: 33 shifted views of the bit stream, 32 mismatch vectors through a
 *           saturating 2-bit counter, then the five shifted q views through a saturating 3-bit counter.
 *   summ    one bit per 32 samples: M is non-zero in this word.  Lets an idle channel be skipped 65536 samples
 *           per step.
 *
 * What stays sequential is the walk from preamble to end flag to preamble: one wave per channel.  SEARCH looks
 * at 2048 samples per step (one M word per lane, one ballot); RECEIVE gathers 64 read positions, one every
 * five samples, per ballot, and does the NRZI decode, the end-flag test, the bit unstuffing and the 1280-bit cut
 * for all 64 at once; kept bits go LSB first into a 160-byte packet in LDS.  The FCS is a CRC-16 (0x8408,
 * reflected) through a 256-entry table in LDS.
 *
 * After a detector reset (stream start, every packet end) the reference's registers and prior_sample slots are
 * zero (:44-50), so for 160 + 4 samples M differs from the free-running map; the walker recomputes those words
 * itself with the pre-reset samples masked off ("EXACT" mode).  The walker's state (including the packet being
 * received) lives on the device between calls, so events do not depend on how a stream is cut into calls.
 */
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/multifm_hip.h"

#include "mfm_bits.h"

extern "C" __attribute__((visibility("hidden"))) void mfm_internal_set_error(const char *msg);

namespace {

constexpr uint32_t AI_HIST = 8192;        /* samples of history kept in front of the newest block (>= 2048 + 192) */
constexpr uint32_t AI_GROUP = 2048;       /* alignment unit: 64 words = one wave of the walker = 2 summary words */
constexpr uint32_t AI_PREAMBLE = 0x5555557eu; /* ais_demod.c:136 */
constexpr uint32_t AI_SLOW_SPAN = 165;    /* samples after a reset during which M differs from the free-running map */
constexpr uint32_t AI_MAX_BITS = 5 * 256; /* ais_demod.c:186 */
constexpr uint32_t AI_PACKET_WORDS = AI_MAX_BITS / 32;

enum : uint32_t { AI_SEARCH = 0, AI_RECEIVE = 1 };

/* ---- bit-sliced preamble correlator --------------------------------------------------------------------- */

/*
 * q word for samples [32 * wi, 32 * wi + 32).  ld(q) returns bit-stream word q (0 for q < 0).  EXACT: samples
 * before r_rel (window-relative index of the reset) read as zero in the slicer history and in the registers,
 * which is what the reference's zero-filled prior_sample slots and preamble registers hold (ais_demod.c:44-50).
 */
template <bool EXACT, class LD>
__device__ __forceinline__ uint32_t ai_q32(LD ld, int32_t wi, int32_t r_rel)
{
    auto mask_before = [&](int32_t P) {
        const int32_t th = r_rel - P; /* samples of the word that lie before the reset */
        return th <= 0 ? 0xffffffffu : (th >= 32 ? 0u : (0xffffffffu << th));
    };
    auto bview = [&](int32_t P) {
        const int32_t q = P >> 5;
        uint32_t x = (P & 31) == 0 ? ld(q) : __builtin_amdgcn_alignbit(ld(q + 1), ld(q), (uint32_t)P & 31u);
        if (EXACT) {
            x &= mask_before(P);
        }
        return x;
    };
    uint32_t s0 = 0, s1 = 0, ov = 0;
    uint32_t cur = bview(32 * wi);
#pragma unroll
    for (int k = 0; k < 32; k++) {
        const int32_t P = 32 * wi - 5 * k;
        const uint32_t prev = bview(P - 5);
        uint32_t n = ~(cur ^ prev); /* ais_demod.c:133 */
        if (EXACT) {
            n &= mask_before(P);
        }
        cur = prev;
        const uint32_t y = ((AI_PREAMBLE >> k) & 1u) ? ~n : n;
        const uint32_t c0 = s0 & y;
        s0 ^= y;
        const uint32_t c1 = s1 & c0;
        s1 ^= c0;
        ov |= c1;
    }
    uint32_t q = ~ov & ~(s0 & s1); /* at most two mismatches (ais_demod.c:40) */
    if (EXACT) {
        q &= mask_before(32 * wi); /* registers not updated since the reset are zero: no match */
    }
    return q;
}

/* M word from the q words of samples [32 wi, 32 wi + 32) and the word before: three or more of five */
__device__ __forceinline__ uint32_t ai_m32(uint32_t qc, uint32_t qp)
{
    uint32_t s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const uint32_t v = j == 0 ? qc : ((qc << j) | (qp >> (32 - j)));
        const uint32_t c0 = s0 & v;
        s0 ^= v;
        const uint32_t c1 = s1 & c0;
        s1 ^= c0;
        s2 |= c1;
    }
    return s2 | (s1 & s0);
}

/* ---- device layout -------------------------------------------------------------------------------------- */

struct AiBuf {
    uint32_t *base; /* planes 0..1 ([plane][channel][BW]) then the summary ([channel][SW]) */
    uint32_t C, BW, SW;
    __host__ __device__ uint32_t *plane(uint32_t p, uint32_t c) const { return base + ((size_t)p * C + c) * BW; }
    __host__ __device__ uint32_t *summ(uint32_t c) const { return base + (size_t)2 * C * BW + (size_t)c * SW; }
};

struct AiChanState {
    uint64_t pos;   /* SEARCH: next sample to look at */
    uint64_t r;     /* SEARCH: first sample after the last detector reset */
    uint64_t rd;    /* RECEIVE: next sample to read a bit from */
    uint64_t start; /* RECEIVE: sample where the preamble matched */
    uint32_t mode, last_sample, hist8, cur_bit;
    uint32_t packet[AI_PACKET_WORDS];
};

/* carry the tail of the window over to the other buffer */
__global__ __launch_bounds__(256) void ai_slide_kernel(AiBuf dst, AiBuf src, uint32_t shift_w, uint32_t keep_w)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t c = blockIdx.y;
    if (k < keep_w) {
        dst.plane(0, c)[k] = src.plane(0, c)[k + shift_w];
        dst.plane(1, c)[k] = src.plane(1, c)[k + shift_w];
    }
    if (k < (keep_w + 31) / 32) {
        dst.summ(c)[k] = src.summ(c)[k + shift_w / 32];
    }
}

/*
 * The slicer: bit = sample > 0 (ais_demod.c:126,172).  HBM-bound: 2 bytes in per sample, 1/8 byte out.  One lane
 * takes 8 consecutive samples with one 16-byte load, squeezes them to a byte, and four neighbouring lanes merge
 * their bytes into a word; a wave covers 512 samples per step and AI_SLICE_U steps are in flight together.
 */
constexpr uint32_t AI_SLICE_U = 4;

struct __attribute__((packed, aligned(2))) AiPcm8 {
    uint32_t d[4];
};

__device__ __forceinline__ uint32_t ai_pos2(uint32_t d)
{
    const int16_t lo = (int16_t)(d & 0xffffu), hi = (int16_t)(d >> 16);
    return (lo > 0 ? 1u : 0u) | (hi > 0 ? 2u : 0u);
}

__global__ __launch_bounds__(256) void ai_slice_kernel(AiBuf buf, const int16_t *x, size_t stride, uint32_t n, uint32_t off0,
                                                      uint32_t nsteps)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t s0 = (blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6)) * AI_SLICE_U;
    const uint32_t c = blockIdx.y;
    if (s0 >= nsteps) {
        return;
    }
    const int16_t *xc = x + (size_t)c * stride;
    const uint32_t base0 = (off0 & ~511u) + 512u * s0 + 8u * lane; /* window-relative index of my first sample */
    uint32_t d[AI_SLICE_U][4];
    const int64_t wave_first = (int64_t)((off0 & ~511u) + 512u * s0) - (int64_t)off0;
    if (wave_first >= 0 && wave_first + 512 * (int64_t)AI_SLICE_U <= (int64_t)n) {
#pragma unroll
        for (uint32_t k = 0; k < AI_SLICE_U; k++) {
            const AiPcm8 v = *reinterpret_cast<const AiPcm8 *>(xc + ((int64_t)base0 + 512 * k - (int64_t)off0));
#pragma unroll
            for (int q = 0; q < 4; q++) {
                d[k][q] = v.d[q];
            }
        }
    } else { /* first / last samples of the call: element by element */
#pragma unroll
        for (uint32_t k = 0; k < AI_SLICE_U; k++) {
            const int64_t i = (int64_t)base0 + 512 * k - (int64_t)off0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int64_t i0 = i + 2 * q, i1 = i0 + 1;
                const uint32_t lo = (i0 >= 0 && i0 < (int64_t)n) ? (uint16_t)xc[i0] : 0u;
                const uint32_t hi = (i1 >= 0 && i1 < (int64_t)n) ? (uint16_t)xc[i1] : 0u;
                d[k][q] = lo | (hi << 16);
            }
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < AI_SLICE_U; k++) {
        uint32_t b = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            b |= ai_pos2(d[k][q]) << (2 * q);
        }
        b |= (uint32_t)__shfl_down((int)b, 1) << 8;
        b |= (uint32_t)__shfl_down((int)b, 2) << 16;
        if (s0 + k < nsteps && (lane & 3u) == 0) {
            const uint32_t first = base0 + 512u * k;
            uint32_t *dst = buf.plane(0, c) + (first >> 5);
            uint32_t word = b;
            if (first < off0) { /* the word straddles the old end: keep the bits that are already there */
                const uint32_t keep = (off0 - first >= 32) ? 0xffffffffu : ((1u << (off0 - first)) - 1u);
                word = (*dst & keep) | (word & ~keep);
            }
            *dst = word;
        }
    }
}

/* free-running M and the summary for words [w_first, w_first + 256 * gridDim.x) */
__global__ __launch_bounds__(256) void ai_match_kernel(AiBuf buf, uint32_t w_first)
{
    constexpr int BACK = 8; /* (160 + 5) samples of register history behind the word before the first one */
    __shared__ uint32_t tile[BACK + 256 + 2];
    __shared__ uint32_t qs[257];
    const uint32_t c = blockIdx.y;
    const int32_t w0 = (int32_t)(w_first + blockIdx.x * 256u);
    const uint32_t *bits = buf.plane(0, c);
    for (int32_t k = (int32_t)threadIdx.x; k < BACK + 256 + 2; k += 256) {
        const int32_t q = w0 - BACK + k;
        tile[k] = q >= 0 ? bits[q] : 0u;
    }
    __syncthreads();
    const int32_t wi = w0 + (int32_t)threadIdx.x;
    auto ld = [&](int32_t q) { return tile[q - (w0 - BACK)]; };
    qs[threadIdx.x + 1] = ai_q32<false>(ld, wi, 0);
    if (threadIdx.x == 0) {
        qs[0] = ai_q32<false>(ld, w0 - 1, 0);
    }
    __syncthreads();
    const uint32_t m = ai_m32(qs[threadIdx.x + 1], qs[threadIdx.x]);
    buf.plane(1, c)[wi] = m;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long any = __ballot(m != 0u);
    if (lane == 0 || lane == 32) {
        buf.summ(c)[(uint32_t)wi >> 5] = (uint32_t)(any >> lane);
    }
}

struct AiWalk {
    AiBuf buf;
    uint64_t ws;  /* absolute sample index of window word 0 */
    uint64_t end; /* absolute index one past the newest sample */
    AiChanState *st;
    mfm_ais_event *ev;
    uint32_t *ev_count;
    uint32_t max_ev;
};

/* one wave per channel: ais_demod_on_pcm (ais_demod.c:215-258) from event to event */
__global__ __launch_bounds__(64) void ai_walk_kernel(const AiWalk L)
{
    __shared__ uint16_t crc_tab[256];
    __shared__ uint32_t pk[AI_PACKET_WORDS];
    const uint32_t lane = threadIdx.x;
    const uint32_t c = blockIdx.x;
    /* CRC-16 table, reflected polynomial 0x8408 (ais_demod.c:19-36) */
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        uint32_t v = lane + 64u * j;
#pragma unroll
        for (int b = 0; b < 8; b++) {
            v = (v & 1u) ? ((v >> 1) ^ 0x8408u) : (v >> 1);
        }
        crc_tab[lane + 64u * j] = (uint16_t)v;
    }
    AiChanState st = L.st[c];
    if (lane < AI_PACKET_WORDS) {
        pk[lane] = st.packet[lane];
    }
    __syncthreads();
    const uint32_t *bits = L.buf.plane(0, c);
    const uint32_t *mplane = L.buf.plane(1, c);
    const uint32_t *summ = L.buf.summ(c);
    mfm_ais_event *ev = L.ev + (size_t)c * L.max_ev;
    uint32_t nev = 0;
    auto getbit = [&](uint64_t n) {
        const uint32_t o = (uint32_t)(n - L.ws);
        return (bits[o >> 5] >> (o & 31u)) & 1u;
    };

    for (;;) {
        if (st.mode == AI_SEARCH) {
            if (st.pos >= L.end) {
                break;
            }
            /* ---- one aligned chunk of 64 words x 32 samples ---- */
            const uint64_t cb = st.pos & ~(uint64_t)(AI_GROUP - 1);
            const int32_t wrel = (int32_t)((cb - L.ws) >> 5) + (int32_t)lane;
            const int64_t lane_base = (int64_t)cb + 32 * (int64_t)lane;
            const int64_t lo64 = (int64_t)st.pos - lane_base, hi64 = (int64_t)L.end - lane_base;
            const int lo = lo64 < 0 ? 0 : (lo64 > 32 ? 32 : (int)lo64);
            const int hi = hi64 < 0 ? 0 : (hi64 > 32 ? 32 : (int)hi64);
            const uint32_t rm = hi > lo ? (((hi == 32) ? 0xffffffffu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u)) : 0u;
            uint32_t m;
            if (cb < st.r + AI_SLOW_SPAN) {
                const int32_t r_rel = (int32_t)((int64_t)st.r - (int64_t)L.ws);
                auto ldg = [&](int32_t q) { return q >= 0 ? bits[q] : 0u; };
                m = ai_m32(ai_q32<true>(ldg, wrel, r_rel), ai_q32<true>(ldg, wrel - 1, r_rel));
            } else {
                m = mplane[wrel];
            }
            m &= rm;
            const unsigned long long hit = __ballot(m != 0u);
            if (hit) {
                /* SEARCH_SYNC -> RECEIVING (ais_demod.c:147-155): first bit read at i + 4, then every 5 samples */
                const int l1 = __ffsll((long long)hit) - 1;
                const uint32_t ml = (uint32_t)__shfl((int)m, l1);
                const uint64_t i = cb + 32u * (uint32_t)l1 + (uint32_t)(__ffs((int)ml) - 1);
                st.mode = AI_RECEIVE;
                st.start = i;
                st.rd = i + 4;
                st.last_sample = getbit(i);
                st.hist8 = 0;
                st.cur_bit = 0;
            } else {
                const uint64_t nxt = cb + AI_GROUP;
                st.pos = nxt < L.end ? nxt : L.end;
                /* past the zero-filled span: jump to the next word with any match in it */
                while (st.pos < L.end && st.pos >= st.r + AI_SLOW_SPAN) {
                    const uint32_t sw0 = (uint32_t)((st.pos - L.ws) >> 10);
                    const uint32_t sidx = sw0 + lane;
                    const uint32_t sv = sidx < L.buf.SW ? summ[sidx] : 0xffffffffu;
                    const unsigned long long nz = __ballot(sv != 0u);
                    if (nz == 0ull) {
                        const uint64_t far = st.pos + 65536ull;
                        st.pos = far < L.end ? far : L.end;
                        continue;
                    }
                    const int l1 = __ffsll((long long)nz) - 1;
                    const uint32_t svw = (uint32_t)__shfl((int)sv, l1);
                    const uint64_t at = L.ws + (((uint64_t)(sw0 + (uint32_t)l1) * 32u + (uint32_t)(__ffs((int)svw) - 1)) << 5);
                    if (at > st.pos) {
                        st.pos = at < L.end ? at : L.end;
                    }
                    break;
                }
            }
        } else {
            /* ---- RECEIVING: 64 bit periods per step (ais_demod.c:160-213) ---- */
            if (st.rd >= L.end) {
                break;
            }
            const uint64_t avail = (L.end - 1 - st.rd) / 5 + 1;
            const uint32_t V = avail < 64 ? (uint32_t)avail : 64u;
            const bool valid = lane < V;
            const uint32_t raw = valid ? getbit(st.rd + 5ull * lane) : 0u;
            uint32_t prev = (uint32_t)__shfl_up((int)raw, 1);
            if (lane == 0) {
                prev = st.last_sample;
            }
            const uint32_t bit = valid ? ((prev ^ raw) ^ 1u) : 0u; /* NRZI: no transition = 1 (:170) */
            const unsigned long long B = __ballot((int)bit);
            /* the eight raw bits ending at mine, oldest in bit 0; hist8 holds those before this step.  raw_shr
             * holds them newest first, but 0x7e reads the same both ways. */
            const uint32_t w = lane >= 7 ? (uint32_t)(B >> (lane - 7)) & 0xffu
                                         : (uint32_t)((B << (7 - lane)) | (unsigned long long)(st.hist8 >> (lane + 1))) & 0xffu;
            const bool flag = valid && w == 0x7eu; /* :186 */
            /* a bit is written only while fewer than five 1s precede it since the rx reset (:175-184); hist8
             * starts at zero at that reset, so "the five bits before are all 1" says the same */
            const bool keep = valid && ((w >> 2) & 31u) != 31u;
            const unsigned long long K = __ballot(keep);
            const uint32_t kept_through = (uint32_t)__popcll(K & ((2ull << lane) - 1ull));
            const bool ends = valid && (flag || st.cur_bit + kept_through >= AI_MAX_BITS);
            const unsigned long long E = __ballot(ends);
            const uint32_t e = E ? (uint32_t)(__ffsll((long long)E) - 1) : V - 1;
            if (keep && bit && lane <= e) {
                const uint32_t p = st.cur_bit + kept_through - 1u; /* < 1280: e is the first lane to reach it */
                atomicOr(&pk[p >> 5], 1u << (p & 31u));
            }
            __syncthreads();
            if (E) {
                const uint32_t nbits = st.cur_bit + (uint32_t)__shfl((int)kept_through, (int)e);
                const uint32_t nr_bytes = nbits / 8u;
                const uint64_t at = st.rd + 5ull * e;
                if (nr_bytes >= 4u) { /* :190-206 */
                    const uint8_t *pb = reinterpret_cast<const uint8_t *>(pk);
                    uint32_t crc = 0xffffu;
                    for (uint32_t k = 0; k < nr_bytes - 2u; k++) {
                        crc = (crc >> 8) ^ crc_tab[(crc ^ pb[k]) & 0xffu];
                    }
                    crc = ~crc & 0xffffu;
                    const uint32_t rx_crc = (uint32_t)pb[nr_bytes - 2u] | ((uint32_t)pb[nr_bytes - 1u] << 8);
                    if (nev < L.max_ev) {
                        mfm_ais_event *o = &ev[nev];
                        if (lane == 0) {
                            o->channel = c;
                            o->fcs_valid = crc == rx_crc ? 1u : 0u;
                            o->nr_bytes = nr_bytes;
                            o->reserved = 0;
                            o->sample = at;
                            o->start_sample = st.start;
                        }
                        if (lane < AI_PACKET_WORDS) {
                            reinterpret_cast<uint32_t *>(o->bytes)[lane] = pk[lane];
                        }
                    }
                    nev++;
                }
                __syncthreads();
                if (lane < AI_PACKET_WORDS) {
                    pk[lane] = 0; /* :53-59 */
                }
                __syncthreads();
                st.mode = AI_SEARCH; /* :207-210: the detector restarts from zero at the next sample */
                st.pos = st.r = at + 1;
            } else {
                st.cur_bit += (uint32_t)__popcll(K);
                st.hist8 = (uint32_t)__shfl((int)w, (int)(V - 1));
                st.last_sample = (uint32_t)__shfl((int)raw, (int)(V - 1));
                st.rd += 5ull * V;
            }
        }
    }
    if (lane < AI_PACKET_WORDS) {
        st.packet[lane] = pk[lane];
    }
    /* every lane holds the whole state; lanes write their share of it */
    AiChanState *dst = &L.st[c];
    if (lane < AI_PACKET_WORDS) {
        dst->packet[lane] = st.packet[lane];
    }
    if (lane == 0) {
        dst->pos = st.pos;
        dst->r = st.r;
        dst->rd = st.rd;
        dst->start = st.start;
        dst->mode = st.mode;
        dst->last_sample = st.last_sample;
        dst->hist8 = st.hist8;
        dst->cur_bit = st.cur_bit;
        L.ev_count[c] = nev;
    }
}

thread_local char g_ai_error[256] = "";

} /* namespace */

#define AI_TRY(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t err_ = (expr);                                                                            \
        if (err_ != hipSuccess) {                                                                            \
            snprintf(g_ai_error, sizeof(g_ai_error), "%s failed: %s", #expr, hipGetErrorString(err_));       \
            mfm_internal_set_error(g_ai_error);                                                              \
            return MFM_E_DEVICE;                                                                             \
        }                                                                                                    \
    } while (0)

struct mfm_ais {
    mfm_ais_config cfg{};
    uint32_t cap_samples = 0, max_ev = 0;
    AiBuf buf[2]{};
    int cur = 0;
    uint64_t ws = 0, total = 0;
    AiChanState *d_st = nullptr;
    mfm_ais_event *d_ev = nullptr;
    uint32_t *d_evcount = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_call = false;
};

extern "C" {

int mfm_ais_create(struct mfm_ais **pp, const struct mfm_ais_config *cfg)
{
    if (!pp || !cfg) {
        return MFM_E_INVAL;
    }
    *pp = nullptr;
    if (cfg->abi_version != MFM_ABI_VERSION || 0 == cfg->nr_channels || 0 == cfg->max_in_samples ||
        cfg->max_in_samples > (1u << 28)) {
        return MFM_E_INVAL;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) {
        return MFM_E_DEVICE; /* no CPU path */
    }
    AI_TRY(hipSetDevice(cfg->device));
    mfm_ais *p = new (std::nothrow) mfm_ais();
    if (!p) {
        return MFM_E_NOMEM;
    }
    p->cfg = *cfg;
    const uint32_t in_round = (cfg->max_in_samples + AI_GROUP - 1) / AI_GROUP * AI_GROUP;
    p->cap_samples = AI_HIST + AI_GROUP + 2 * in_round;
    p->max_ev = cfg->max_events ? cfg->max_events : cfg->max_in_samples / 160 + 16;
    const uint32_t BW = p->cap_samples / 32 + 256 + 8; /* the match kernel rounds its range up to 256 words */
    const uint32_t SW = BW / 32 + 4;
    const uint32_t C = cfg->nr_channels;
    *pp = p;
    for (int i = 0; i < 2; i++) {
        const size_t bytes = ((size_t)2 * C * BW + (size_t)C * SW) * 4;
        p->buf[i] = AiBuf{ nullptr, C, BW, SW };
        AI_TRY(hipMalloc(&p->buf[i].base, bytes));
        AI_TRY(hipMemset(p->buf[i].base, 0, bytes));
    }
    AI_TRY(hipMalloc(&p->d_st, (size_t)C * sizeof(AiChanState)));
    AI_TRY(hipMemset(p->d_st, 0, (size_t)C * sizeof(AiChanState))); /* SEARCH at sample 0, reset at 0 */
    AI_TRY(hipMalloc(&p->d_ev, (size_t)C * p->max_ev * sizeof(mfm_ais_event)));
    AI_TRY(hipMalloc(&p->d_evcount, (size_t)C * 4));
    AI_TRY(hipMemset(p->d_evcount, 0, (size_t)C * 4));
    AI_TRY(hipDeviceSynchronize());
    return MFM_OK;
}

void mfm_ais_destroy(struct mfm_ais **pp)
{
    if (!pp || !*pp) {
        return;
    }
    mfm_ais *p = *pp;
    (void)hipSetDevice(p->cfg.device);
    (void)hipDeviceSynchronize();
    (void)hipFree(p->buf[0].base);
    (void)hipFree(p->buf[1].base);
    (void)hipFree(p->d_st);
    (void)hipFree(p->d_ev);
    (void)hipFree(p->d_evcount);
    delete p;
    *pp = nullptr;
}

} /* extern "C" */

/* the head of a process call, whichever way the bits arrive: order the call behind the last one, make room for n samples
 * (slide) and say where in the window they go */
static int ai_begin(mfm_ais *p, uint32_t n, hipStream_t s, uint32_t *poff0)
{
    const uint32_t C = p->cfg.nr_channels;
    AI_TRY(hipSetDevice(p->cfg.device));
    if (p->have_call && p->last_stream != s) {
        AI_TRY(hipStreamSynchronize(p->last_stream)); /* state lives on the device; keep calls ordered */
    }
    uint32_t off0 = (uint32_t)(p->total - p->ws);
    if ((uint64_t)off0 + n > p->cap_samples) {
        const uint64_t new_ws = (p->total & ~(uint64_t)(AI_GROUP - 1)) - AI_HIST;
        const uint32_t shift_w = (uint32_t)((new_ws - p->ws) >> 5);
        const uint32_t used_w = ((off0 + 31) / 32 + 63) / 64 * 64;
        const uint32_t keep_w = used_w - shift_w;
        hipLaunchKernelGGL(ai_slide_kernel, dim3((keep_w + 255) / 256, C), dim3(256), 0, s, p->buf[p->cur ^ 1], p->buf[p->cur],
                           shift_w, keep_w);
        AI_TRY(hipGetLastError());
        p->cur ^= 1;
        p->ws = new_ws;
        off0 = (uint32_t)(p->total - p->ws);
    }
    *poff0 = off0;
    return MFM_OK;
}

/* the tail of a process call, once bits [off0, off0 + n) of plane 0 are in place: match, walk, bookkeeping */
static int ai_finish(mfm_ais *p, uint32_t n, uint32_t off0, hipStream_t s)
{
    const uint32_t C = p->cfg.nr_channels;
    const AiBuf buf = p->buf[p->cur];
    if (n) {
        const uint32_t w_first = (off0 & ~(AI_GROUP - 1)) / 32;
        const uint32_t w_end = (off0 + n + 31) / 32;
        hipLaunchKernelGGL(ai_match_kernel, dim3((w_end - w_first + 255) / 256, C), dim3(256), 0, s, buf, w_first);
        AI_TRY(hipGetLastError());
    }
    AiWalk W{ buf, p->ws, p->total + n, p->d_st, p->d_ev, p->d_evcount, p->max_ev };
    hipLaunchKernelGGL(ai_walk_kernel, dim3(C), dim3(64), 0, s, W);
    AI_TRY(hipGetLastError());
    p->total += n;
    p->last_stream = s;
    p->have_call = true;
    return MFM_OK;
}

extern "C" {

int mfm_ais_process_device(struct mfm_ais *p, const int16_t *d_pcm, size_t in_stride, size_t nr_in, void *stream)
{
    if (!p || (!d_pcm && nr_in) || nr_in > p->cfg.max_in_samples) {
        return MFM_E_INVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t C = p->cfg.nr_channels, n = (uint32_t)nr_in;
    uint32_t off0 = 0;
    const int rc = ai_begin(p, n, s, &off0);
    if (rc != MFM_OK) {
        return rc;
    }
    if (n) {
        const uint32_t nsteps = (off0 + n - (off0 & ~511u) + 511) / 512;
        hipLaunchKernelGGL(ai_slice_kernel, dim3((nsteps + 4 * AI_SLICE_U - 1) / (4 * AI_SLICE_U), C), dim3(256), 0, s, p->buf[p->cur],
                           d_pcm, in_stride, n, off0, nsteps);
        AI_TRY(hipGetLastError());
    }
    return ai_finish(p, n, off0, s);
}

int mfm_ais_process_bits_device(struct mfm_ais *p, const struct mfm_bits_view *view, void *stream)
{
    if (!p || !view || (!view->d_bits && view->nr_bits) || view->nr_bits > p->cfg.max_in_samples) {
        return MFM_E_INVAL;
    }
    if (view->polarity != MFM_BITS_POS) {
        snprintf(g_ai_error, sizeof(g_ai_error), "the AIS stage slices with sample > 0: it takes MFM_BITS_POS views (got polarity %u)",
                 view->polarity);
        mfm_internal_set_error(g_ai_error);
        return MFM_E_INVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t C = p->cfg.nr_channels, n = (uint32_t)view->nr_bits;
    uint32_t off0 = 0;
    const int rc = ai_begin(p, n, s, &off0);
    if (rc != MFM_OK) {
        return rc;
    }
    if (n) {
        /* the words the slicer writes: from the one that holds off0 to the end of the call's last group of 512 samples */
        const uint32_t w0 = off0 >> 5, nw = ((off0 + n + 511u) & ~511u) / 32u - w0;
        const AiBuf buf = p->buf[p->cur];
        hipLaunchKernelGGL(mfm_splice_kernel, dim3((nw + 255) / 256, C), dim3(256), 0, s, buf.plane(0, 0), buf.BW, view->d_bits,
                           view->stride_words, n, off0, w0, nw);
        AI_TRY(hipGetLastError());
    }
    return ai_finish(p, n, off0, s);
}

int mfm_ais_process_host(struct mfm_ais *p, const int16_t *pcm, size_t in_stride, size_t nr_in)
{
    if (!p || (!pcm && nr_in)) {
        return MFM_E_INVAL;
    }
    AI_TRY(hipSetDevice(p->cfg.device));
    const uint32_t C = p->cfg.nr_channels;
    int16_t *d_in = nullptr;
    AI_TRY(hipMalloc(&d_in, (size_t)C * (nr_in ? nr_in : 1) * 2));
    if (nr_in) {
        AI_TRY(hipMemcpy2D(d_in, nr_in * 2, pcm, in_stride * 2, nr_in * 2, C, hipMemcpyHostToDevice));
    }
    const int rc = mfm_ais_process_device(p, d_in, nr_in, nr_in, nullptr);
    (void)hipDeviceSynchronize();
    (void)hipFree(d_in);
    return rc;
}

int mfm_ais_seek(struct mfm_ais *p, uint64_t samples_before)
{
    if (!p) {
        mfm_internal_set_error("mfm_ais_seek: no object");
        return MFM_E_INVAL;
    }
    if (samples_before >= (1ull << 62)) {
        mfm_internal_set_error("mfm_ais_seek: samples_before must stay below 2^62 (the walk forms int64 differences of positions)");
        return MFM_E_INVAL;
    }
    AI_TRY(hipSetDevice(p->cfg.device));
    if (p->have_call) {
        AI_TRY(hipStreamSynchronize(p->last_stream));
    }
    /* what create leaves, with the window's word 0 on the group that holds samples_before: the bits in front of it are
     * zero, and the detector reset lies on it */
    const uint32_t C = p->cfg.nr_channels;
    std::vector<AiChanState> st(C);
    memset(st.data(), 0, (size_t)C * sizeof(AiChanState));
    for (uint32_t c = 0; c < C; c++) {
        st[c].mode = AI_SEARCH;
        st[c].pos = st[c].r = samples_before;
    }
    for (int i = 0; i < 2; i++) {
        AI_TRY(hipMemset(p->buf[i].base, 0, ((size_t)2 * C * p->buf[i].BW + (size_t)C * p->buf[i].SW) * 4));
    }
    AI_TRY(hipMemcpy(p->d_st, st.data(), (size_t)C * sizeof(AiChanState), hipMemcpyHostToDevice));
    AI_TRY(hipMemset(p->d_evcount, 0, (size_t)C * 4));
    AI_TRY(hipDeviceSynchronize());
    p->cur = 0;
    p->ws = samples_before & ~(uint64_t)(AI_GROUP - 1);
    p->total = samples_before;
    p->last_stream = nullptr;
    p->have_call = false;
    return MFM_OK;
}

int mfm_ais_fetch_events(struct mfm_ais *p, struct mfm_ais_event *out, size_t max_events, size_t *nr_events)
{
    if (!p || !nr_events || (!out && max_events)) {
        return MFM_E_INVAL;
    }
    *nr_events = 0;
    if (!p->have_call) {
        return MFM_OK;
    }
    AI_TRY(hipSetDevice(p->cfg.device));
    AI_TRY(hipStreamSynchronize(p->last_stream));
    const uint32_t C = p->cfg.nr_channels;
    std::vector<uint32_t> cnt(C);
    AI_TRY(hipMemcpy(cnt.data(), p->d_evcount, (size_t)C * 4, hipMemcpyDeviceToHost));
    size_t total = 0;
    bool overflow = false;
    for (uint32_t c = 0; c < C; c++) {
        overflow |= cnt[c] > p->max_ev;
        total += cnt[c] > p->max_ev ? p->max_ev : cnt[c];
    }
    *nr_events = total;
    if (total > max_events) {
        return MFM_E_NOMEM;
    }
    size_t pos = 0;
    for (uint32_t c = 0; c < C; c++) {
        const uint32_t k = cnt[c] > p->max_ev ? p->max_ev : cnt[c];
        if (k) {
            AI_TRY(hipMemcpy(out + pos, p->d_ev + (size_t)c * p->max_ev, (size_t)k * sizeof(mfm_ais_event), hipMemcpyDeviceToHost));
            pos += k;
        }
    }
    if (overflow) {
        snprintf(g_ai_error, sizeof(g_ai_error), "a channel produced more than max_events=%u events in one call", p->max_ev);
        mfm_internal_set_error(g_ai_error);
        return MFM_E_STATE;
    }
    return MFM_OK;
}

} /* extern "C" */
