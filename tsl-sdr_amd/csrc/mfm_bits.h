/*
 * mfm_bits.h - the sign-bit path between the resampler and the POCSAG / AIS stages: how a call's packed predicate bits
 * (struct mfm_bits_view, include/multifm_hip.h) are spliced into a stage's bit window in the place of its slicer.
 *
 * Both stages keep plane 0 of their window as [channel][BW] words, bit b of the window = bit b % 32 of word b / 32,
 * and the newest sample of the previous calls sits just below window bit off0.  The source is aligned to the call
 * (output j = bit j), so window word w takes source bits [32 w - off0, 32 w - off0 + 32): a funnel shift of two source
 * words.  The word that straddles off0 keeps what is below it; bits at and above off0 + nr_bits are zero, as the
 * slicers' element-by-element edge path writes them (the match kernels read those words).
 *
 * mfm_splice_word() is the one statement of that arithmetic: the kernel below runs it per word on the GPU,
 * mfm_hosttwin_splice_bits() runs it on the host, where the CPU tests compare it with a numpy restatement.
 */
#ifndef MFM_BITS_H
#define MFM_BITS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* what window word w holds after the splice; `old` is what it held before (only used where the word starts below off0) */
__host__ __device__ inline uint32_t mfm_splice_word(const uint32_t *src, uint64_t nr_bits, uint64_t off0, uint64_t w, uint32_t old)
{
    const uint64_t first = 32u * w, end = off0 + nr_bits, nw = (nr_bits + 31u) / 32u;
    if (first + 32u <= off0) {
        return old; /* wholly older than this call */
    }
    uint32_t v, keep = 0;
    if (first >= off0) {
        const uint64_t k = (first - off0) >> 5;
        const uint32_t sh = (uint32_t)(first - off0) & 31u;
        const uint32_t lo = k < nw ? src[k] : 0u, hi = k + 1u < nw ? src[k + 1u] : 0u;
        v = sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
    } else { /* the word straddles the old end: keep the bits that are already there */
        const uint32_t s = (uint32_t)(off0 - first); /* 1 .. 31 */
        v = (nw ? src[0] : 0u) << s;
        keep = (1u << s) - 1u;
    }
    if (first + 32u > end) { /* zeros from the end of the call on, whatever the source holds behind its last bit */
        v &= end > first ? (1u << (uint32_t)(end - first)) - 1u : 0u;
    }
    return (old & keep) | (v & ~keep);
}

/*
 * The splice in the place of pg_slice_kernel / ai_slice_kernel: words [w0, w0 + nw) of plane 0, one lane per word.
 * The caller passes w0 = off0 / 32 and runs nw up to the next multiple of 512 samples behind the call's end - the
 * words the slicers write.  HBM: 1/8 byte in and 1/8 byte out per sample.
 */
static __global__ __launch_bounds__(256) void mfm_splice_kernel(uint32_t *plane0, uint32_t bw, const uint32_t *src, size_t stride_words,
                                                               uint32_t nr_bits, uint32_t off0, uint32_t w0, uint32_t nw)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t c = blockIdx.y;
    if (k >= nw) {
        return;
    }
    const uint32_t w = w0 + k;
    uint32_t *dst = plane0 + (size_t)c * bw + w;
    const uint32_t old = 32u * w < off0 ? *dst : 0u;
    *dst = mfm_splice_word(src + (size_t)c * stride_words, nr_bits, off0, w, old);
}

#endif /* MFM_BITS_H */
