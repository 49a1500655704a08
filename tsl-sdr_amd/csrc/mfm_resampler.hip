/*
 * mfm_resampler.hip - the PCM stage behind the channel FIFOs, batched over all channels on the GPU:
 * real-valued rational resampler (filter/polyphase_fir.c, filter/utils.c) and DC blocker
 * (filter/dc_blocker.h).  See include/multifm_hip.h for the boundary and the reference lines.
 *
 * Kernel shape: grid = (blocks of 1024 outputs, channels).  All channels share the phase walk (they receive the
 * same number of samples), so output j of a call starts at sample (p0 + j*D) / I with phase (p0 + j*D) % I.
 * A workgroup copies the input window of its 1024 outputs (about 1024 * D / I + phase length samples) into LDS -
 * straight from where the samples lie: the unconsumed tail of the previous call (a few dozen samples per channel,
 * ping-pong buffers) followed by the caller's PCM, no staging copy - and every thread computes 4 outputs as
 * v_dot2_i32_i16 over sample pairs (int32 wrap-around like filter/utils.c:94-103; an odd window start costs one
 * funnel shift per pair).  When 256 * D is a multiple of I - 4/5 for POCSAG, 16/25 for FLEX - a thread's four
 * outputs share one phase and its coefficient pairs stay in registers; otherwise they are read from LDS.
 * HBM traffic: 2 bytes in + 2 * I / D bytes out per PCM sample.
 *
 * Matrix-core form (round 2; used when 16 D / I is an integer - 4/5 and 16/25 both - and the window fits 256 bytes).
 * The v_dot2 form is bound by the vector ALU, not by memory: 16/25 with the reference's 821 taps is 26 coefficient
 * pairs = 78 instructions per output, 0.11 ms per block for 64 channels where the channel kernel in front of it takes
 * 0.125.  Sixteen consecutive outputs consume exactly R = 16 D / I samples and their phases repeat from block to
 * block, so  y[16 m + q] = sum_s G[q][s] x[R m + s]  with ONE 16 x K matrix G (row q = the phase of output q shifted
 * to where its window starts, zero elsewhere; one G per value of the carried phase) - a GEMM with M = 16 = the matrix
 * instruction's M, columns = blocks of 16 outputs.  int16 x int16 -> wrapping int32 is done exactly as in the channel
 * kernel (mfm_kernel_mfma.hip): W = 256 Wh + Wl, x = 256 Xh + Xl + 128, four v_mfma_i32_16x16x64_i8 per 64 elements.
 * The input lies in LDS as two byte planes in rows of R samples padded to 16-byte multiples (zero coefficients over
 * the padding), so that a lane's B operand is one aligned ds_read_b128: the window of block m is rows m, m+1, ...
 * A lane ends up with four consecutive outputs of one block: one 8-byte store.
 * The DC blocker is a sequential IIR with a truncating shift in the loop (not associative): one thread
 * per channel.
 *
 * Sign-bit form of the output (mfm_resampler_process_bits_device).  The POCSAG and AIS stages reduce every resampled sample
 * to one predicate (< 0, > 0), so both kernels have a second epilogue, chosen at compile time (template argument BITS; 0 is
 * the PCM epilogue, unchanged), that takes the predicate of the Q14-rounded value in registers and stores packed words
 * instead of PCM: 1/8 byte per output instead of 2, and nothing for a slicer to read back.
 *   v_dot2 form: the lanes of a wave hold 64 consecutive outputs per step, so __ballot(predicate) is two finished words.
 *   matrix form: a lane (kg, n) holds a nibble, outputs 16 n + 4 kg + i of the 256 consecutive outputs of its wave's column
 *   group g, i.e. bits 16 (n & 1) + 4 kg of word n / 2 of that run.  The four groups' nibbles are merged over kg with a
 *   reduce-scatter (lane bits 5 and 4: three cross-lane moves for the four groups, after which lane (kg, n) holds group
 *   g = kg) and over n & 1 with one more; the even lanes then hold the wave's 32 words in order: one 128-byte store per wave.
 *
 * Which kernel runs: decided by rs_plan() (mfm_rs_plan.h) on the host, before the first HIP call, from I, D, the taps and
 * the flags alone; mfm_resampler_get_form() reports it and tests/test_resampler_forms.py pins it.  The rules, in the order the
 * planner applies them:
 *   [plen]   phase length = ceil(taps / I), rounded up to a multiple of 4 (filter/polyphase_fir.c:70-83)
 *   [walk]   refused (MFM_E_INVAL): ceil(D / I) > plen - an output would consume more samples than a phase holds
 *   [range]  refused: max_out * D >= 2^32 - the phase walk of a call is 32-bit arithmetic in the kernels
 *   [lds]    LDS of a v_dot2 workgroup = 2 I plen (coefficient pairs) + 2 (floor(1024 D / I) + plen + 32) (the window of 1024
 *            outputs) bytes, rounded up to 16; refused above 150 KB, whichever form would run
 *   [np]     v_dot2 instance: the coefficient pairs in registers when 256 D % I == 0 (a thread's four outputs share a phase),
 *            plen / 2 <= 32 and that LDS is at most 48 KB - NP = plen / 2 rounded up to 4, one of 4, 8, ..., 32; else NP = 0, pairs
 *            read from LDS.  Above 48 KB create raises the NP = 0 kernels' dynamic LDS limit
 *            (hipFuncAttributeMaxDynamicSharedMemorySize)
 *   [matrix] the matrix form unless, first reason that applies (mfm_resampler_form::fallback):
 *              forced     MFM_RS_FORCE_DOT2
 *              ratio      16 D / I is not an integer
 *              block      R = 16 D / I > 240
 *              window     K > 256, where K = (last / R) rp + last % R + 1 rounded up to 64 is the length in bytes of a block's
 *                         window in rows of R samples padded to rp = R rounded up to 16, last = floor((I - 1 + 15 D) / I) + plen - 1
 *              tap range  a tap beyond +-32639 (does not split into two signed bytes)
 *            with KS = K / 64 k-steps (1 .. 4) and 2 planes of (256 + ceil(K / rp)) rp bytes of LDS, each rounded up to 64: up to
 *            123 904 bytes (1/15).  Observed on an MI355X with this runtime (HIP 7.2): launches of this kernel with 66 048, 82 560
 *            and 123 904 bytes of dynamic LDS are accepted and bit-exact without raising its limit first, so create does not
 *            raise it
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

namespace {

struct RsLaunch {
    const int16_t *tail;  /* [C][tail_cap]: what the previous call left unconsumed */
    const int16_t *pcm;   /* [C][in_stride]: this call's samples, where the caller has them */
    int16_t *y;           /* [C][out_cap] */
    const int16_t *phase; /* [I][plen] */
    int16_t *tail_out;    /* [C][tail_cap]: what this call leaves unconsumed (mfm_rs_tail_kernel) */
    size_t in_stride;
    uint32_t tail_len, nr_in, tail_cap, out_cap, n_out, plen, interp, decim, p0, nchan, invert;
    uint32_t pos_end, new_tail;
    uint32_t *bits;       /* sign-bit form: [C][bits_stride] words, output j = bit j % 32 of word j / 32 */
    uint32_t bits_stride;
};

/* the predicate of the sign-bit forms, on the Q14-rounded output as the PCM form stores it: cut to int16 (utils.c:112 - a
 * sum beyond the int16 range wraps, and the stages see the wrapped sample) */
template <int BITS>
__device__ __forceinline__ bool rs_pred(int32_t y)
{
    const int16_t s = (int16_t)y;
    return BITS == (int)MFM_BITS_NEG ? s < 0 : s > 0;
}

/* sample v of channel c in the virtual stream "tail, then the new samples"; decoder -i negates on int16 storage */
__device__ __forceinline__ int16_t rs_sample(const RsLaunch &L, uint32_t c, uint32_t v)
{
    int16_t s = 0;
    if (v < L.tail_len) {
        s = L.tail[(size_t)c * L.tail_cap + v];
    } else if (v - L.tail_len < L.nr_in) {
        s = L.pcm[(size_t)c * L.in_stride + (v - L.tail_len)];
    }
    return L.invert ? (int16_t)(-s) : s; /* decoder.c:624: samp[i] *= -1 */
}

/* NP > 0: coefficient pairs of the thread's phase in registers, NP = pairs per phase rounded up to a multiple of 4
 * (the padding pairs are zero); NP = 0: pairs read from LDS, any phase length */
template <int NP, int BITS>
__global__ __launch_bounds__(RS_NT) void mfm_resample_kernel(const RsLaunch L)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t rs_smem[];
    uint32_t *ph_s = reinterpret_cast<uint32_t *>(rs_smem);                 /* [I][plen / 2] coefficient pairs */
    const uint32_t npairs = L.plen / 2u;                                     /* plen is a multiple of 4 */
    int16_t *x_s = reinterpret_cast<int16_t *>(rs_smem + (size_t)L.interp * L.plen * 2u);
    const uint32_t c = blockIdx.y, tid = threadIdx.x;
    const uint32_t j0 = blockIdx.x * RS_OPB;
    const uint32_t j1 = (j0 + RS_OPB < L.n_out ? j0 + RS_OPB : L.n_out) - 1u; /* last output of the block */
    /* filter/polyphase_fir.c:206-211 unrolled to output j: position (p0 + j D) / I, phase (p0 + j D) % I */
    /* p0 + j D fits 32 bits for every output of a call (create() checks out_cap * D < 2^32) */
    const uint32_t in_lo = ((L.p0 + j0 * L.decim) / L.interp) & ~1u;
    const uint32_t in_hi = (L.p0 + j1 * L.decim) / L.interp + L.plen + 2u + 8u; /* + the zero-padded pairs */
    for (uint32_t i = tid; i < L.interp * npairs; i += RS_NT) {
        ph_s[i] = reinterpret_cast<const uint32_t *>(L.phase)[i];
    }
    for (uint32_t v = in_lo + tid; v < in_hi; v += RS_NT) {
        x_s[v - in_lo] = rs_sample(L, c, v);
    }
    __syncthreads();
    const uint32_t *x32 = reinterpret_cast<const uint32_t *>(x_s);

    /* one division per thread: its outputs are RS_NT apart, so position and phase advance by constants */
    const uint32_t t_first = L.p0 + (j0 + tid) * L.decim;
    uint32_t pos_abs = t_first / L.interp, ph = t_first - pos_abs * L.interp;
    const uint32_t step_pos = (RS_NT * L.decim) / L.interp, step_ph = (RS_NT * L.decim) % L.interp;
    constexpr bool REGCOEF = NP > 0;
    uint32_t cw[REGCOEF ? NP : 1];
    if (REGCOEF) {
        /* 256 * D is a multiple of I: outputs tid, tid + 256, ... of this block have the same phase */
#pragma unroll
        for (uint32_t i = 0; i < (uint32_t)NP; i++) {
            cw[i] = i < npairs ? ph_s[ph * npairs + i] : 0u;
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < RS_OPT; u++) {
        const uint32_t j = j0 + tid + u * RS_NT;
        if (j >= L.n_out) {
            break;
        }
        const uint32_t pos = pos_abs - in_lo;
        const uint32_t *xw = x32 + (pos >> 1);
        const uint32_t sh = (pos & 1u) * 16u;
        int32_t acc = 0; /* filter/utils.c:94-103, int32 wrap-around */
        uint32_t lo = xw[0];
        if (REGCOEF) {
#pragma unroll
            for (uint32_t i = 0; i < (uint32_t)NP; i++) {
                const uint32_t hi = xw[i + 1];
                const uint32_t pr = __builtin_amdgcn_alignbit(hi, lo, sh); /* samples pos + 2i, pos + 2i + 1 */
                asm("v_dot2_i32_i16 %0, %1, %2, %0" : "+v"(acc) : "v"(pr), "v"(cw[i]));
                lo = hi;
            }
        } else {
            const uint32_t *cp = ph_s + ph * npairs;
            for (uint32_t i = 0; i < npairs; i++) {
                const uint32_t hi = xw[i + 1];
                const uint32_t pr = __builtin_amdgcn_alignbit(hi, lo, sh);
                asm("v_dot2_i32_i16 %0, %1, %2, %0" : "+v"(acc) : "v"(pr), "v"(cp[i]));
                lo = hi;
            }
        }
        asm volatile("s_nop 2" : "+v"(acc)); /* a DOT result needs 3 wait states before other VALU code reads it */
        if (BITS) {
            /* outputs j0 + 256 u + 64 wave + lane: the wave's active lanes (those below n_out; lane 0 is one of them) hold the
             * bits of two consecutive words, the lanes that left the loop count as 0 */
            const unsigned long long m = __ballot(rs_pred<BITS>(mfm_r14_wide(acc)));
            if ((tid & 31u) == 0) {
                L.bits[(size_t)c * L.bits_stride + (j >> 5)] = (uint32_t)(m >> (tid & 32u));
            }
        } else {
            L.y[(size_t)c * L.out_cap + j] = (int16_t)mfm_r14_wide(acc); /* utils.c:112 */
        }
        pos_abs += step_pos;
        ph += step_ph;
        if (ph >= L.interp) {
            ph -= L.interp;
            pos_abs += 1u;
        }
    }
}

/* what this call leaves unconsumed: samples pos_end .. pos_end + new_tail of the virtual stream (new_tail <= plen) */
__global__ void mfm_rs_tail_kernel(const RsLaunch L)
{
    const uint32_t c = blockIdx.x;
    for (uint32_t i = threadIdx.x; i < L.new_tail; i += blockDim.x) {
        int16_t s = 0;
        const uint32_t v = L.pos_end + i;
        if (v < L.tail_len) {
            s = L.tail[(size_t)c * L.tail_cap + v];
        } else if (v - L.tail_len < L.nr_in) {
            s = L.pcm[(size_t)c * L.in_stride + (v - L.tail_len)];
        }
        L.tail_out[(size_t)c * L.tail_cap + i] = s; /* stored as received: inversion is applied on use */
    }
}

/* ---- matrix-core form ------------------------------------------------------------------------------------- */

typedef int rs_v4i __attribute__((ext_vector_type(4)));

struct RsMLaunch {
    RsLaunch b;
    const rs_v4i *gfrag; /* [2 planes: Wh, Wl][KS][64 lanes] A fragments of G for this call's carried phase */
    const int32_t *krow; /* [16]: 128 * sum of row q of G (the x = ... + 128 term) */
    uint32_t R;          /* samples per block of 16 outputs = 16 D / I */
    uint32_t rp;         /* bytes per row in LDS: R rounded up to a multiple of 16 */
    uint32_t plane;      /* bytes per byte plane in LDS */
};

struct __attribute__((packed, aligned(2))) RsPcm8 {
    int16_t v[8];
};

template <int KS, int BITS>
__global__ __launch_bounds__(RSM_NT) void mfm_resample_mfma_kernel(const RsMLaunch M)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t rs_smem[];
    const RsLaunch &L = M.b;
    uint8_t *const pl_h = rs_smem, *const pl_l = rs_smem + M.plane;
    const uint32_t c = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t b0 = blockIdx.x * RSM_NB;                  /* first block of this workgroup */
    const uint32_t nrows = RSM_NB + (64u * KS + M.rp - 1u) / M.rp; /* image rows: the last block's window is 64 KS bytes long */
    const uint32_t v0 = b0 * M.R;

    /* ---- stage: a work item = eight samples of one row, as two 8-byte LDS writes (one per byte plane).  The last
     * group of a row runs into the padding (8 ceil(R / 8) <= rp) and carries the next row's first samples there -
     * G is zero over the padding ---- */
    const uint32_t g8 = (M.R + 7u) / 8u;                       /* groups per row */
    for (uint32_t it = tid; it < nrows * g8; it += RSM_NT) {
        const uint32_t row = it / g8, grp = it - row * g8;
        const uint32_t v = v0 + row * M.R + 8u * grp;
        uint32_t w[4];
        if (v >= L.tail_len && v + 8u <= L.tail_len + L.nr_in) {
            const RsPcm8 p = *reinterpret_cast<const RsPcm8 *>(L.pcm + (size_t)c * L.in_stride + (v - L.tail_len));
#pragma unroll
            for (int i = 0; i < 4; i++) {
                w[i] = mfm_pack16(p.v[2 * i], p.v[2 * i + 1]);
            }
            if (L.invert) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    w[i] = mfm_pack16(-(int32_t)p.v[2 * i], -(int32_t)p.v[2 * i + 1]); /* decoder.c:624 on int16 storage */
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) { /* the tail of the previous call, the seam, zeros past the end */
                w[i] = mfm_pack16(rs_sample(L, c, v + 2u * (uint32_t)i), rs_sample(L, c, v + 2u * (uint32_t)i + 1u));
            }
        }
        uint2 lo, hi;
        lo.x = __builtin_amdgcn_perm(w[1], w[0], 0x06040200u) ^ 0x80808080u; /* Xl = (x & 255) - 128 */
        lo.y = __builtin_amdgcn_perm(w[3], w[2], 0x06040200u) ^ 0x80808080u;
        hi.x = __builtin_amdgcn_perm(w[1], w[0], 0x07050301u);                /* Xh = x >> 8 */
        hi.y = __builtin_amdgcn_perm(w[3], w[2], 0x07050301u);
        const uint32_t at = row * M.rp + 8u * grp;
        *reinterpret_cast<uint2 *>(pl_l + at) = lo;
        *reinterpret_cast<uint2 *>(pl_h + at) = hi;
    }
    __syncthreads();

    /* ---- multiply: lane (kg, n) reads 16 bytes of column (block) n at element 64 ks + 16 kg ---- */
    const uint32_t kg = lane >> 4, n = lane & 15u;
    rs_v4i a_h[KS], a_l[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
        a_h[ks] = M.gfrag[(0 * KS + ks) * 64 + lane];
        a_l[ks] = M.gfrag[(1 * KS + ks) * 64 + lane];
    }
    rs_v4i kr;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        kr[i] = M.krow[4u * kg + (uint32_t)i];
    }
    uint32_t nibw[4] = { 0, 0, 0, 0 }; /* sign-bit form: my nibble of column group g, at its place in its word */
#pragma unroll
    for (uint32_t g = 0; g < 4; g++) {
        const uint32_t blk = wave * 64u + g * 16u + n;          /* block within the workgroup */
        const uint32_t off = blk * M.rp + 16u * kg;
        rs_v4i hh = { 0, 0, 0, 0 }, md = hh, ll = hh;
#pragma unroll
        for (int ks = 0; ks < KS; ks++) {
            const rs_v4i b_h = *reinterpret_cast<const rs_v4i *>(pl_h + off + 64u * ks);
            const rs_v4i b_l = *reinterpret_cast<const rs_v4i *>(pl_l + off + 64u * ks);
            hh = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_h[ks], b_h, hh, 0, 0, 0);
            md = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_h[ks], b_l, md, 0, 0, 0);
            ll = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_l[ks], b_l, ll, 0, 0, 0);
            md = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_l[ks], b_h, md, 0, 0, 0);
        }
        /* rows 4 kg .. 4 kg + 3 of column n = outputs 16 (b0 + blk) + 4 kg + i */
        const uint32_t j = 16u * (b0 + blk) + 4u * kg;
        int32_t y[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t acc = (uint32_t)ll[i] + ((uint32_t)md[i] << 8) + ((uint32_t)hh[i] << 16) + (uint32_t)kr[i];
            y[i] = mfm_r14_wide((int32_t)acc); /* utils.c:112 */
        }
        if (BITS) {
            uint32_t nib = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                nib |= (rs_pred<BITS>(y[i]) && j + (uint32_t)i < L.n_out ? 1u : 0u) << i;
            }
            nibw[g] = nib << (16u * (n & 1u) + 4u * kg);
            continue;
        }
        int16_t *dst = L.y + (size_t)c * L.out_cap + j;
        if (j + 4u <= L.n_out) {
            uint2 w;
            w.x = mfm_pack16(y[0], y[1]);
            w.y = mfm_pack16(y[2], y[3]);
            *reinterpret_cast<uint2 *>(dst) = w; /* out_cap and j are multiples of 4: 8-byte aligned */
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (j + (uint32_t)i < L.n_out) {
                    dst[i] = (int16_t)y[i];
                }
            }
        }
    }
    if (BITS) {
        /* OR over kg = lane bits 5, 4, handing one half of what is left to the partner at each step: 2 + 1 moves, after
         * which lane (kg, n) holds the nibbles of all kg for group g = kg; then over n & 1 */
        const bool b5 = (lane & 32u) != 0u, b4 = (lane & 16u) != 0u;
        uint32_t k0 = b5 ? nibw[2] : nibw[0], k1 = b5 ? nibw[3] : nibw[1];
        k0 |= (uint32_t)__shfl_xor((int)(b5 ? nibw[0] : nibw[2]), 32);
        k1 |= (uint32_t)__shfl_xor((int)(b5 ? nibw[1] : nibw[3]), 32);
        uint32_t k = b4 ? k1 : k0;
        k |= (uint32_t)__shfl_xor((int)(b4 ? k0 : k1), 16);
        k |= (uint32_t)__shfl_xor((int)k, 1);
        /* word n / 2 of group kg: outputs 16 (b0 + 64 wave + 16 kg) + 32 (n / 2) ..., i.e. the wave's 32 words in lane order */
        const uint32_t wi = (b0 >> 1) + 32u * wave + 8u * kg + (n >> 1);
        if ((n & 1u) == 0u && 32u * wi < L.n_out) {
            L.bits[(size_t)c * L.bits_stride + wi] = k;
        }
    }
}

struct DcState {
    int32_t x_n_1, y_n_1, acc;
};

/*
 * filter/dc_blocker.h:80-90, one lane per channel.  The loop is a feedback loop with a truncating shift inside (not
 * associative, and two trajectories that start apart take ~2^14 / p samples to meet, so there is nothing to split in
 * time): what can be done is to keep the per-sample work down to the recurrence itself.  With acc_n = (x_n << 14) + r_n
 * the reference's four statements are  r_n = r_(n-1) - p y_(n-1),  y_n = (int32)((x_n << 14) + r_n) >> 14  (all mod
 * 2^32, as the reference's int32 arithmetic wraps); samples are read and written eight at a time (16-byte accesses, the
 * next eight requested before the current eight are worked on), so a sample costs a few instructions instead of a global
 * load - store round trip (94 ms -> 6.2 ms per 447 392-sample block in round 2; 5.8 ms with the three-instruction chain of
 * round 5).  What bounds it now is the chain itself: y -> multiply-add -> multiply-add -> shift -> y is three dependent
 * instructions, 26 cycles per sample as measured, and one wave of 64 channels has nothing to put in between; a second
 * formulation with a chain of two (u_n = y_(n-1) * -p + (u_(n-1) + dX_n), y_n = u_n >> 14) needs five instructions per
 * sample and would land at ~4.3 ms.  The (Y, r) form (acc = 2^14 Y + r) has the same chain length as this one.  Off by
 * default in the reference (decoder -b), not on multifm's path.
 */
__global__ __launch_bounds__(64) void mfm_dc_block_kernel(int16_t *y, uint32_t out_cap, uint32_t n_out, uint32_t nchan, int32_t p,
                                                          DcState *st)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchan) {
        return;
    }
    const DcState s0 = st[c];
    /* r = acc - x_(n-1) << 14 in the reference's variables */
    uint32_t r = (uint32_t)s0.acc - (uint32_t)s0.x_n_1;
    int32_t yp = s0.y_n_1, xl = 0;
    int16_t *yy = y + (size_t)c * out_cap;
    uint32_t i = 0;
    /* 64 samples per trip: the next 64 are requested (eight 16-byte loads in flight) before the current 64 are worked
     * on - a lane's row is its own cache lines, so a load that is waited for costs a full memory round trip */
    constexpr uint32_t V = 8;
    if (n_out >= 8u * V) {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4))); /* (HIP's uint4 is a struct of unions: arrays of it end up in scratch) */
        const u32x4 *src = reinterpret_cast<const u32x4 *>(yy); /* out_cap is a multiple of 8: rows are 16-byte aligned */
        u32x4 *dst = reinterpret_cast<u32x4 *>(yy);
        u32x4 cur[V], nxt[V];
#pragma unroll
        for (uint32_t k = 0; k < V; k++) {
            cur[k] = src[k];
        }
        const int32_t np = -p; /* |p| < 2^15 and |y| <= 2^17: the products fit the 24-bit multiplier (one v_mad_i32_i24) */
        for (; i + 8u * V <= n_out; i += 8u * V) {
            /* the next 64 samples; behind the last whole group the same ones again (a valid address, nobody uses them) */
            const u32x4 *pn = src + (i + 16u * V <= n_out ? i / 8u + V : i / 8u);
#pragma unroll
            for (uint32_t k = 0; k < V; k++) {
                nxt[k] = pn[k];
            }
#pragma unroll
            for (uint32_t k = 0; k < V; k++) {
                const u32x4 w = cur[k];
                u32x4 o;
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    /* three instructions per sample on the chain y -> r -> acc -> y (round 5; five before): the multiply-add of
                     * the leak, (x << 14) + r as ONE v_mad_i32_i16 that picks the sample's half of the packed word itself
                     * (x * 16384 + r, wrapping like the reference's int32), the arithmetic shift; half a v_perm to pack */
                    uint32_t acc;
                    r += (uint32_t)__mul24(yp, np);
                    asm("v_mad_i32_i16 %0, %1, %2, %3 op_sel:[0,0,0,0]" : "=v"(acc) : "v"(w[d]), "s"(16384), "v"(r));
                    yp = (int32_t)acc >> 14;
                    const uint32_t lo = (uint32_t)yp;
                    r += (uint32_t)__mul24(yp, np);
                    asm("v_mad_i32_i16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(acc) : "v"(w[d]), "s"(16384), "v"(r));
                    yp = (int32_t)acc >> 14;
                    o[d] = __builtin_amdgcn_perm((uint32_t)yp, lo, 0x05040100u); /* low halves of (lo, yp) */
                }
                xl = (int32_t)w[3] >> 16; /* the group's last sample: x_(n-1) of whatever follows */
                dst[i / 8u + k] = o;
            }
#pragma unroll
            for (uint32_t k = 0; k < V; k++) {
                cur[k] = nxt[k];
            }
        }
    }
    for (; i < n_out; i++) {
        r -= (uint32_t)p * (uint32_t)yp;
        xl = (int32_t)yy[i];
        yp = (int32_t)(((uint32_t)xl << 14) + r) >> 14;
        yy[i] = (int16_t)yp;
    }
    if (n_out) {
        DcState s;
        s.x_n_1 = (int32_t)((uint32_t)xl << 14);
        s.acc = (int32_t)(((uint32_t)xl << 14) + r);
        s.y_n_1 = yp;
        st[c] = s;
    }
}

thread_local char g_rs_error[256] = "";

} /* namespace */

struct mfm_resampler {
    mfm_resampler_config cfg{};
    RsPlan plan; /* what create() decided (mfm_rs_plan.h); the fields below that repeat it are what the launches read */
    uint32_t plen = 0;
    uint32_t in_cap = 0, out_cap = 0;
    int16_t *d_phase = nullptr;
    int16_t *d_x[2] = { nullptr, nullptr }; /* [C][tail_cap] ping-pong: the samples the last call left unconsumed */
    uint32_t tail_cap = 0;
    uint32_t lds_bytes = 0;
    bool reg_coef = false;
    int16_t *d_y = nullptr;
    DcState *d_dc = nullptr;
    int32_t dc_p = 0;
    int cur = 0;
    uint32_t tail = 0; /* unconsumed samples in d_x[cur] */
    uint32_t phase_id = 0;
    int16_t *d_stage = nullptr; /* process_host_to_device: [C][max_in_samples] */
    uint32_t *d_bits = nullptr; /* sign-bit form: [C][bits_stride], allocated by the first bits call */
    uint32_t bits_stride = 0;
    /* matrix-core form */
    bool use_mfma = false;
    uint32_t m_ks = 0, m_R = 0, m_rp = 0, m_plane = 0, m_lds = 0;
    rs_v4i *d_gfrag = nullptr; /* [I][2][KS][64] */
    int32_t *d_krow = nullptr; /* [I][16] */
};

#define RS_TRY(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t err_ = (expr);                                                                            \
        if (err_ != hipSuccess) {                                                                            \
            snprintf(g_rs_error, sizeof(g_rs_error), "%s failed: %s", #expr, hipGetErrorString(err_));       \
            mfm_internal_set_error(g_rs_error);                                                              \
            return MFM_E_DEVICE;                                                                             \
        }                                                                                                    \
    } while (0)

extern "C" {

int mfm_resampler_create(struct mfm_resampler **pr, const struct mfm_resampler_config *cfg, const int16_t *coeffs,
                         size_t nr_coeffs)
{
    if (!pr || !cfg || !coeffs || 0 == nr_coeffs) {
        return MFM_E_INVAL;
    }
    *pr = nullptr;
    if (!rs_args_ok(*cfg, nr_coeffs)) {
        return MFM_E_INVAL;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) {
        return MFM_E_DEVICE; /* no CPU path */
    }
    mfm_resampler *r = new (std::nothrow) mfm_resampler();
    if (!r) {
        return MFM_E_NOMEM;
    }
    r->cfg = *cfg;
    /* everything that is decided is decided here, on the host (mfm_rs_plan.h) ... */
    RsPlan &p = r->plan;
    const int rc = rs_plan(*cfg, coeffs, nr_coeffs, p);
    if (rc != MFM_OK) {
        if (p.err[0]) {
            mfm_internal_set_error(p.err);
        }
        delete r;
        return rc;
    }
    RsTables t;
    rs_build_tables(p, coeffs, t);
    r->plen = p.plen;
    r->in_cap = p.in_cap;
    r->out_cap = p.out_cap;
    r->tail_cap = p.tail_cap;
    r->dc_p = p.dc_p;
    r->lds_bytes = p.lds_bytes;
    r->reg_coef = p.reg_coef;
    r->use_mfma = p.use_mfma;
    r->m_ks = p.ks;
    r->m_R = p.R;
    r->m_rp = p.rp;
    r->m_plane = p.m_plane;
    r->m_lds = p.m_lds;
    /* ... what follows allocates and uploads */
    *pr = r;
    RS_TRY(hipSetDevice(cfg->device));
    RS_TRY(hipMalloc(&r->d_phase, t.phase.size() * 2));
    RS_TRY(hipMemcpy(r->d_phase, t.phase.data(), t.phase.size() * 2, hipMemcpyHostToDevice));
    for (int i = 0; i < 2; i++) {
        RS_TRY(hipMalloc(&r->d_x[i], (size_t)cfg->nr_channels * r->tail_cap * 2));
        RS_TRY(hipMemset(r->d_x[i], 0, (size_t)cfg->nr_channels * r->tail_cap * 2));
    }
    if (!p.use_mfma && p.lds_bytes > RS_LDS_DEFAULT) {
        RS_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(mfm_resample_kernel<0, 0>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)r->lds_bytes));
        RS_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(mfm_resample_kernel<0, (int)MFM_BITS_NEG>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)r->lds_bytes));
        RS_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(mfm_resample_kernel<0, (int)MFM_BITS_POS>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)r->lds_bytes));
    }
    if (p.use_mfma) {
        RS_TRY(hipMalloc(&r->d_gfrag, t.frag.size()));
        RS_TRY(hipMemcpy(r->d_gfrag, t.frag.data(), t.frag.size(), hipMemcpyHostToDevice));
        RS_TRY(hipMalloc(&r->d_krow, t.krow.size() * 4));
        RS_TRY(hipMemcpy(r->d_krow, t.krow.data(), t.krow.size() * 4, hipMemcpyHostToDevice));
    }
    RS_TRY(hipMalloc(&r->d_y, (size_t)cfg->nr_channels * r->out_cap * 2));
    RS_TRY(hipMalloc(&r->d_dc, (size_t)cfg->nr_channels * sizeof(DcState)));
    RS_TRY(hipMemset(r->d_dc, 0, (size_t)cfg->nr_channels * sizeof(DcState)));
    RS_TRY(hipDeviceSynchronize());
    return MFM_OK;
}

void mfm_resampler_destroy(struct mfm_resampler **pr)
{
    if (!pr || !*pr) {
        return;
    }
    mfm_resampler *r = *pr;
    (void)hipSetDevice(r->cfg.device);
    (void)hipDeviceSynchronize();
    (void)hipFree(r->d_phase);
    (void)hipFree(r->d_x[0]);
    (void)hipFree(r->d_x[1]);
    (void)hipFree(r->d_y);
    (void)hipFree(r->d_dc);
    (void)hipFree(r->d_stage);
    (void)hipFree(r->d_bits);
    (void)hipFree(r->d_gfrag);
    (void)hipFree(r->d_krow);
    delete r;
    *pr = nullptr;
}

size_t mfm_resampler_max_out(const struct mfm_resampler *r)
{
    return r ? r->out_cap : 0;
}

int mfm_resampler_get_form(const struct mfm_resampler *r, struct mfm_resampler_form *form)
{
    if (!r || !form) {
        return MFM_E_INVAL;
    }
    rs_plan_form(r->plan, form);
    return MFM_OK;
}

int mfm_hosttwin_resampler_form(const struct mfm_resampler_config *cfg, const int16_t *coeffs, size_t nr_coeffs,
                                struct mfm_resampler_form *form)
{
    if (!cfg || !coeffs || !form) {
        return MFM_E_INVAL;
    }
    RsPlan p;
    const int rc = rs_plan(*cfg, coeffs, nr_coeffs, p);
    if (rc != MFM_OK) {
        mfm_internal_set_error(p.err[0] ? p.err : "invalid resampler configuration");
        return rc;
    }
    rs_plan_form(p, form);
    return MFM_OK;
}

int mfm_hosttwin_resampler_matrix_block(const struct mfm_resampler_config *cfg, const int16_t *coeffs, size_t nr_coeffs,
                                        uint32_t phase, const int16_t *x, size_t nr_x, int16_t y16[16])
{
    if (!cfg || !coeffs || (!x && nr_x) || !y16) {
        return MFM_E_INVAL;
    }
    RsPlan p;
    const int rc = rs_plan(*cfg, coeffs, nr_coeffs, p);
    if (rc != MFM_OK || !p.use_mfma || phase >= p.I) {
        return MFM_E_INVAL;
    }
    RsTables t;
    rs_build_tables(p, coeffs, t);
    /* the LDS image of one block's window: K bytes of rows of R samples padded to rp, as the staging loop of
     * mfm_resample_mfma_kernel leaves them (Xl = (x & 255) - 128, Xh = x >> 8); nothing defined is in the padding */
    std::vector<int8_t> pl_h(p.K, 0x55), pl_l(p.K, 0x55);
    for (uint32_t kk = 0; kk < p.K; kk++) {
        const uint32_t row = kk / p.rp, col = kk % p.rp;
        if (col < p.R) {
            const size_t v = (size_t)row * p.R + col;
            const int32_t s = v < nr_x ? x[v] : 0;
            pl_l[kk] = (int8_t)((s & 0xff) ^ 0x80);
            pl_h[kk] = (int8_t)(s >> 8);
        }
    }
    /* lane (kg, n) of the kernel: column n is this block; its A fragment is row i = lane & 15 of G, its results rows 4 kg .. 4 kg + 3.
     * Row q of the product sums, per k-step, the 16 elements of each of the four lanes (kgq, q) against bytes 64 ks + 16 kgq + j. */
    const int8_t *a_h = t.frag.data() + ((size_t)phase * 2u + 0u) * p.ks * 64u * 16u;
    const int8_t *a_l = t.frag.data() + ((size_t)phase * 2u + 1u) * p.ks * 64u * 16u;
    for (uint32_t q = 0; q < 16; q++) {
        uint32_t hh = 0, md = 0, ll = 0;
        for (uint32_t ks = 0; ks < p.ks; ks++) {
            for (uint32_t kgq = 0; kgq < 4; kgq++) {
                const size_t fa = ((size_t)ks * 64u + kgq * 16u + q) * 16u;
                const uint32_t off = 16u * kgq + 64u * ks;
                for (uint32_t j = 0; j < 16; j++) {
                    const int32_t ah = a_h[fa + j], al = a_l[fa + j], bh = pl_h[off + j], bl = pl_l[off + j];
                    hh += (uint32_t)(ah * bh);
                    md += (uint32_t)(ah * bl) + (uint32_t)(al * bh);
                    ll += (uint32_t)(al * bl);
                }
            }
        }
        const uint32_t acc = ll + (md << 8) + (hh << 16) + (uint32_t)t.krow[(size_t)phase * 16u + q];
        y16[q] = (int16_t)mfm_r14_wide((int32_t)acc); /* utils.c:112 */
    }
    return MFM_OK;
}

} /* extern "C" */

/* one call of either output form: BITS = 0 writes PCM to d_y, MFM_BITS_NEG / MFM_BITS_POS the packed predicate to d_bits.
 * The walk, the carried tail and the phase are the same, so the two forms may alternate on one stream. */
template <int BITS>
static int rs_process(mfm_resampler *r, const int16_t *d_pcm, size_t in_stride, size_t nr_in, hipStream_t s, uint32_t *pn_out)
{
    const uint32_t C = r->cfg.nr_channels, I = r->cfg.interpolate, D = r->cfg.decimate;
    const uint32_t total = r->tail + (uint32_t)nr_in;
    /* outputs m with total - pos_m > plen  <=>  p0 + m*D < (total - plen) * I   (polyphase_fir.c:184) */
    uint32_t n_out = 0;
    if (total > r->plen) {
        const uint64_t lim = (uint64_t)(total - r->plen) * I;
        if (lim > r->phase_id) {
            n_out = (uint32_t)((lim - r->phase_id + D - 1) / D);
        }
    }
    const uint64_t t_end = (uint64_t)r->phase_id + (uint64_t)n_out * D;
    const uint32_t pos_end = (uint32_t)(t_end / I);
    /* pos_end <= total (create() checked ceil(D/I) <= plen) and total - pos_end <= plen: with outputs, t_end >= (total -
     * plen) * I; without, total <= plen */
    const uint32_t new_tail = total - pos_end;
    RsLaunch L{ r->d_x[r->cur], d_pcm, r->d_y, r->d_phase, r->d_x[r->cur ^ 1], in_stride, r->tail, (uint32_t)nr_in, r->tail_cap,
                r->out_cap, n_out, r->plen, I, D, r->phase_id, C, r->cfg.invert, pos_end, new_tail, r->d_bits, r->bits_stride };
    if (n_out && r->use_mfma) {
        RsMLaunch M{ L, r->d_gfrag + (size_t)r->phase_id * 2u * r->m_ks * 64u, r->d_krow + (size_t)r->phase_id * 16u, r->m_R, r->m_rp,
                     r->m_plane };
        const dim3 grid((n_out + 16u * RSM_NB - 1u) / (16u * RSM_NB), C);
        switch (r->m_ks) {
        case 1: hipLaunchKernelGGL((mfm_resample_mfma_kernel<1, BITS>), grid, dim3(RSM_NT), r->m_lds, s, M); break;
        case 2: hipLaunchKernelGGL((mfm_resample_mfma_kernel<2, BITS>), grid, dim3(RSM_NT), r->m_lds, s, M); break;
        case 3: hipLaunchKernelGGL((mfm_resample_mfma_kernel<3, BITS>), grid, dim3(RSM_NT), r->m_lds, s, M); break;
        default: hipLaunchKernelGGL((mfm_resample_mfma_kernel<4, BITS>), grid, dim3(RSM_NT), r->m_lds, s, M); break;
        }
        RS_TRY(hipGetLastError());
    } else if (n_out) {
        const dim3 grid((n_out + RS_OPB - 1) / RS_OPB, C);
        const uint32_t np4 = r->reg_coef ? (r->plen / 2u + 3u) / 4u : 0u; /* register variant: pairs rounded up to 4 */
        switch (np4) {
        case 1: hipLaunchKernelGGL((mfm_resample_kernel<4, BITS>), grid, dim3(RS_NT), r->lds_bytes, s, L); break;
        case 2: hipLaunchKernelGGL((mfm_resample_kernel<8, BITS>), grid, dim3(RS_NT), r->lds_bytes, s, L); break;
        case 3: hipLaunchKernelGGL((mfm_resample_kernel<12, BITS>), grid, dim3(RS_NT), r->lds_bytes, s, L); break;
        case 4: hipLaunchKernelGGL((mfm_resample_kernel<16, BITS>), grid, dim3(RS_NT), r->lds_bytes, s, L); break;
        case 5: hipLaunchKernelGGL((mfm_resample_kernel<20, BITS>), grid, dim3(RS_NT), r->lds_bytes, s, L); break;
        case 6: hipLaunchKernelGGL((mfm_resample_kernel<24, BITS>), grid, dim3(RS_NT), r->lds_bytes, s, L); break;
        case 7: hipLaunchKernelGGL((mfm_resample_kernel<28, BITS>), grid, dim3(RS_NT), r->lds_bytes, s, L); break;
        case 8: hipLaunchKernelGGL((mfm_resample_kernel<32, BITS>), grid, dim3(RS_NT), r->lds_bytes, s, L); break;
        default: hipLaunchKernelGGL((mfm_resample_kernel<0, BITS>), grid, dim3(RS_NT), r->lds_bytes, s, L); break;
        }
        RS_TRY(hipGetLastError());
    }
    if (n_out && !BITS) {
        if (r->cfg.dc_block) {
            hipLaunchKernelGGL(mfm_dc_block_kernel, dim3((C + 63) / 64), dim3(64), 0, s, r->d_y, r->out_cap, n_out, C,
                               r->dc_p, r->d_dc);
            RS_TRY(hipGetLastError());
        }
    }
    if (new_tail) {
        hipLaunchKernelGGL(mfm_rs_tail_kernel, dim3(C), dim3(64), 0, s, L);
        RS_TRY(hipGetLastError());
    }
    r->phase_id = (uint32_t)(t_end % I);
    r->tail = new_tail;
    r->cur ^= 1;
    *pn_out = n_out;
    return MFM_OK;
}

/* what every bits call checks before it touches the stream position; allocates the bit rows on first use */
static int rs_bits_prepare(mfm_resampler *r, uint32_t polarity)
{
    if (polarity != MFM_BITS_NEG && polarity != MFM_BITS_POS) {
        snprintf(g_rs_error, sizeof(g_rs_error), "unknown sign-bit polarity %u (MFM_BITS_NEG or MFM_BITS_POS)", polarity);
        mfm_internal_set_error(g_rs_error);
        return MFM_E_INVAL;
    }
    if (r->cfg.dc_block) {
        snprintf(g_rs_error, sizeof(g_rs_error), "the sign-bit output is not available with the DC blocker: it filters the "
                                                 "resampled PCM in memory, which this form does not write");
        mfm_internal_set_error(g_rs_error);
        return MFM_E_INVAL;
    }
    RS_TRY(hipSetDevice(r->cfg.device));
    if (!r->d_bits) {
        /* a matrix-form wave stores 32 words at once and checks only its own word against n_out: rows of whole words */
        r->bits_stride = ((r->out_cap + 31u) / 32u + 7u) & ~7u;
        RS_TRY(hipMalloc(&r->d_bits, (size_t)r->cfg.nr_channels * r->bits_stride * 4));
    }
    return MFM_OK;
}

extern "C" {

int mfm_resampler_process_device(struct mfm_resampler *r, const int16_t *d_pcm, size_t in_stride, size_t nr_in,
                                 void *stream, int16_t **d_out, size_t *out_stride, size_t *nr_out)
{
    if (!r || !d_pcm || !d_out || !out_stride || !nr_out) {
        return MFM_E_INVAL;
    }
    if (nr_in > r->cfg.max_in_samples) {
        return MFM_E_INVAL;
    }
    RS_TRY(hipSetDevice(r->cfg.device));
    uint32_t n_out = 0;
    const int rc = rs_process<0>(r, d_pcm, in_stride, nr_in, static_cast<hipStream_t>(stream), &n_out);
    if (rc != MFM_OK) {
        return rc;
    }
    *d_out = r->d_y;
    *out_stride = r->out_cap;
    *nr_out = n_out;
    return MFM_OK;
}

int mfm_resampler_process_bits_device(struct mfm_resampler *r, const int16_t *d_pcm, size_t in_stride, size_t nr_in,
                                      void *stream, uint32_t polarity, struct mfm_bits_view *view)
{
    if (!r || !d_pcm || !view || nr_in > r->cfg.max_in_samples) {
        return MFM_E_INVAL;
    }
    int rc = rs_bits_prepare(r, polarity);
    if (rc != MFM_OK) {
        return rc;
    }
    uint32_t n_out = 0;
    rc = polarity == MFM_BITS_NEG ? rs_process<(int)MFM_BITS_NEG>(r, d_pcm, in_stride, nr_in, static_cast<hipStream_t>(stream), &n_out)
                                  : rs_process<(int)MFM_BITS_POS>(r, d_pcm, in_stride, nr_in, static_cast<hipStream_t>(stream), &n_out);
    if (rc != MFM_OK) {
        return rc;
    }
    view->d_bits = r->d_bits;
    view->stride_words = r->bits_stride;
    view->nr_bits = n_out;
    view->polarity = polarity;
    view->reserved = 0;
    return MFM_OK;
}

int mfm_resampler_process_host_to_device(struct mfm_resampler *r, const int16_t *pcm, size_t in_stride, size_t nr_in,
                                         void *stream, int16_t **d_out, size_t *out_stride, size_t *nr_out)
{
    if (!r || (!pcm && nr_in) || nr_in > r->cfg.max_in_samples) {
        return MFM_E_INVAL;
    }
    RS_TRY(hipSetDevice(r->cfg.device));
    const uint32_t C = r->cfg.nr_channels;
    if (!r->d_stage) {
        RS_TRY(hipMalloc(&r->d_stage, (size_t)C * r->cfg.max_in_samples * 2));
    }
    if (nr_in) {
        RS_TRY(hipMemcpy2DAsync(r->d_stage, (size_t)r->cfg.max_in_samples * 2, pcm, in_stride * 2, nr_in * 2, C,
                                hipMemcpyHostToDevice, static_cast<hipStream_t>(stream)));
    }
    return mfm_resampler_process_device(r, r->d_stage, r->cfg.max_in_samples, nr_in, stream, d_out, out_stride, nr_out);
}

int mfm_resampler_process_bits_host_to_device(struct mfm_resampler *r, const int16_t *pcm, size_t in_stride, size_t nr_in,
                                              void *stream, uint32_t polarity, struct mfm_bits_view *view)
{
    if (!r || (!pcm && nr_in) || !view || nr_in > r->cfg.max_in_samples) {
        return MFM_E_INVAL;
    }
    const int rc = rs_bits_prepare(r, polarity); /* refuse before anything is staged */
    if (rc != MFM_OK) {
        return rc;
    }
    const uint32_t C = r->cfg.nr_channels;
    if (!r->d_stage) {
        RS_TRY(hipMalloc(&r->d_stage, (size_t)C * r->cfg.max_in_samples * 2));
    }
    if (nr_in) {
        RS_TRY(hipMemcpy2DAsync(r->d_stage, (size_t)r->cfg.max_in_samples * 2, pcm, in_stride * 2, nr_in * 2, C,
                                hipMemcpyHostToDevice, static_cast<hipStream_t>(stream)));
    }
    return mfm_resampler_process_bits_device(r, r->d_stage, r->cfg.max_in_samples, nr_in, stream, polarity, view);
}

int mfm_resampler_process_host(struct mfm_resampler *r, const int16_t *pcm, size_t in_stride, size_t nr_in,
                               int16_t *out, size_t out_stride, size_t *nr_out)
{
    if (!r || !pcm || !out || !nr_out) {
        return MFM_E_INVAL;
    }
    RS_TRY(hipSetDevice(r->cfg.device));
    int16_t *d_in = nullptr;
    const uint32_t C = r->cfg.nr_channels;
    RS_TRY(hipMalloc(&d_in, (size_t)C * (nr_in ? nr_in : 1) * 2));
    if (nr_in) {
        RS_TRY(hipMemcpy2D(d_in, nr_in * 2, pcm, in_stride * 2, nr_in * 2, C, hipMemcpyHostToDevice));
    }
    int16_t *d_out = nullptr;
    size_t ostr = 0, n = 0;
    int rc = mfm_resampler_process_device(r, d_in, nr_in, nr_in, nullptr, &d_out, &ostr, &n);
    if (rc == MFM_OK && n) {
        if (n > out_stride) {
            rc = MFM_E_INVAL;
        } else {
            hipError_t e = hipMemcpy2D(out, out_stride * 2, d_out, ostr * 2, n * 2, C, hipMemcpyDeviceToHost);
            if (e != hipSuccess) {
                rc = MFM_E_DEVICE;
            }
        }
    }
    (void)hipDeviceSynchronize();
    (void)hipFree(d_in);
    *nr_out = n;
    return rc;
}

int mfm_resampler_process_bits_host(struct mfm_resampler *r, const int16_t *pcm, size_t in_stride, size_t nr_in,
                                    uint32_t polarity, uint32_t *bits, size_t bits_stride_words, size_t *nr_bits)
{
    if (!r || !pcm || !bits || !nr_bits) {
        return MFM_E_INVAL;
    }
    int rc = rs_bits_prepare(r, polarity);
    if (rc != MFM_OK) {
        return rc;
    }
    int16_t *d_in = nullptr;
    const uint32_t C = r->cfg.nr_channels;
    RS_TRY(hipMalloc(&d_in, (size_t)C * (nr_in ? nr_in : 1) * 2));
    if (nr_in) {
        RS_TRY(hipMemcpy2D(d_in, nr_in * 2, pcm, in_stride * 2, nr_in * 2, C, hipMemcpyHostToDevice));
    }
    mfm_bits_view v{};
    rc = mfm_resampler_process_bits_device(r, d_in, nr_in, nr_in, nullptr, polarity, &v);
    const size_t nw = (v.nr_bits + 31u) / 32u;
    if (rc == MFM_OK && nw) {
        if (nw > bits_stride_words) {
            rc = MFM_E_INVAL;
        } else {
            hipError_t e = hipMemcpy2D(bits, bits_stride_words * 4, v.d_bits, v.stride_words * 4, nw * 4, C, hipMemcpyDeviceToHost);
            if (e != hipSuccess) {
                rc = MFM_E_DEVICE;
            }
        }
    }
    (void)hipDeviceSynchronize();
    (void)hipFree(d_in);
    *nr_bits = v.nr_bits;
    return rc;
}

} /* extern "C" */
