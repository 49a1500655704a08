/*
 * mfm_plan.hip - the channel engine's kernel plan (mfm_plan.h): which kernel form runs a channel set, its geometry, its
 * launch descriptions, and the host tables it reads.  Host code only; the kernel files' select functions it asks are table
 * lookups over template instances.
 */
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>

#include "mfm_plan.h"
#include "mfm_numerics.h"

extern "C" hipError_t mfm_select_channel_kernel(int opl, int dbg_iq, const void **kfn_out);
extern "C" hipError_t mfm_select_channel_kernel_mfma(const mfm_launch_mfma *L, int dbg_iq, const void **kfn_out,
                                                     uint32_t *waves_per_simd_out);
extern "C" hipError_t mfm_select_channel_kernel_v3(const mfm_launch_v3 *L, int dbg_iq, const void **kfn_out);
extern "C" uint32_t mfm_rot_entry_bytes_v3(void);
extern "C" uint32_t mfm_sp_pitch_v3(void);
extern "C" uint32_t mfm_v3l_wg_per_cu(const mfm_launch_v3 *L);
extern "C" __attribute__((visibility("hidden"))) void mfm_internal_set_error(const char *msg);

namespace {

constexpr uint32_t kMaxOutputsPerTile = 128;
/* 128-tap filters: slices of 128 channels from this many channels on (below, slices of 64: MFM_F_SLICE_128 / _64 override) */
constexpr uint32_t kSlice128MinChannels = 512; /* the measured crossover (profiles/r06_slice128_ab.txt): +1.8 % at 128, +1.7 % at 256,
                                                 -0.6 % at 512, -0.8 % at 768, -1.4 % at 1024 channels */
/* second-generation kernels: PCM stores with system scope from this many channels per launch on (profiles/r05_store_policy.txt,
 * r06_hbm_traffic_1024ch.json: L2-miss traffic 1.27 -> 1.16 x algorithmic at 1024 channels at unchanged time; +0.4 % time at 256
 * channels and 1.5-5 % at 64, where there is nothing to gain: profiles/r06_ab_store_policy.txt) */
constexpr uint32_t kPcmWriteThroughMinChannels = 512;
constexpr uint64_t kMaxRotEntries = 1ull << 26; /* per distinct increment: 512 MiB of table */

int fail(int code, const char *fmt, ...)
{
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    mfm_internal_set_error(msg);
    return code;
}

/* LDS row stride: an ODD multiple of 32 bytes.  tools/ubench_lds.hip: the B-fragment read pattern (lane 16 kg + n reads 16
 * bytes at n * rs + 16 kg) runs at the full ds_read_b128 rate for rs = 224 and at 76-81 % of it for 80, 144, 176, 192, 208,
 * 272 - odd multiples of 16 bytes are not enough. */
uint32_t odd32_stride(uint32_t row_bytes)
{
    const uint32_t rs = (row_bytes + 31u) / 32u * 32u;
    return ((rs / 32u) & 1u) ? rs : rs + 32u;
}

/* element index of the last tap + 1 of a window whose LDS rows are row_bytes plane bytes (2 D of samples, then padding) */
uint32_t window_elems(uint32_t T, uint32_t D, uint32_t row_bytes)
{
    return ((T - 1u) / D) * row_bytes + 2u * ((T - 1u) % D) + 2u;
}

/* k-steps (64 elements) whose high-byte tap plane is not all zero: a window's elements of tap i are (cr, -ci) and (ci, cr)
 * (filter/complex.h:40-46), each split into 256 * high + low with both signed bytes */
uint32_t tap_plane_mask(const std::vector<Channel> &chans, uint32_t T, uint32_t D, uint32_t row_bytes)
{
    uint32_t mask = 0;
    for (const Channel &ch : chans) {
        for (uint32_t i = 0; i < T; i++) {
            const uint32_t kst = ((i / D) * row_bytes + 2u * (i % D)) / 64u;
            for (int32_t w : { (int32_t)ch.cre[i], (int32_t)ch.cim[i], -(int32_t)ch.cim[i] }) {
                const int32_t wl = (int8_t)(w & 0xff);
                if (((w - wl) >> 8) != 0) {
                    mask |= 1u << kst;
                }
            }
        }
    }
    return mask;
}

/* the order the long-filter kernel multiplies the k-steps in (mfm_launch_v3::kperm): those with a high-byte tap plane first,
 * then the others that hold taps, then - up to the instance's count - steps of zero taps */
void kstep_order(uint32_t hi_mask, uint32_t kq_used, uint32_t kq_inst, uint32_t kperm[4])
{
    uint8_t order[16] = { 0 };
    uint32_t at = 0;
    for (uint32_t k = 0; k < kq_used; k++) {
        if ((hi_mask >> k) & 1u) {
            order[at++] = (uint8_t)k;
        }
    }
    for (uint32_t k = 0; k < kq_inst; k++) {
        if (!((hi_mask >> k) & 1u)) {
            order[at++] = (uint8_t)k;
        }
    }
    for (int w = 0; w < 4; w++) {
        kperm[w] = (uint32_t)order[4 * w] | ((uint32_t)order[4 * w + 1] << 8) | ((uint32_t)order[4 * w + 2] << 16) |
                   ((uint32_t)order[4 * w + 3] << 24);
    }
}

/* decimations 1, 2, 4 (etc/multifm_file.json: 1): rows shorter than a fragment - the long-filter kernel keeps 8 / D shifted
 * copies of the image instead of padding them (mfm_kernel_v3l.hip, SHIFT); the window is then the unpadded 2 T elements */
bool shift_geometry(const KernelPlan &p, uint32_t flags)
{
    return (1u == p.D || 2u == p.D || 4u == p.D) && p.T <= 512u && !(flags & (MFM_F_FORCE_MFMA_V1 | MFM_F_FORCE_DOT2));
}

/* [dot2] the v_dot2 kernel: two outputs per lane where the tile fits 53 KiB of LDS, else one */
int plan_dot2(KernelPlan &p)
{
    const uint32_t T = p.T, D = p.D;
    const uint32_t qrows = (T + D - 1) / D;
    auto tile_dwords = [&](int opl, uint32_t *rs2) {
        const uint32_t rows = 64u * opl - 1u + qrows;
        *rs2 = rows | 1u; /* odd stride: transposing stores hit 32 different banks */
        return (uint64_t)D * *rs2;
    };
    uint32_t rs2 = 0;
    int opl = 2;
    uint64_t dw = tile_dwords(2, &rs2);
    if ((dw + 512) * 4 > 53 * 1024) {
        opl = 1;
        dw = tile_dwords(1, &rs2);
    }
    if ((dw + 512) * 4 > 160 * 1024) {
        return fail(MFM_E_INVAL, "decimation %u needs a %llu-byte LDS tile (> 160 KiB)", D, (unsigned long long)(dw + 512) * 4);
    }
    p.opl = opl;
    p.rs2 = rs2;
    p.lut_off = (uint32_t)((dw + 3) & ~3ull);
    p.lds_bytes = (p.lut_off + 512) * 4;
    p.nchunks = (T + MFM_TG - 1) / MFM_TG;
    p.ngroups = (p.C + MFM_CG - 1) / MFM_CG;
    p.gpw = std::min<uint32_t>(MFM_NW, p.ngroups);
    p.nslices = (p.ngroups + p.gpw - 1) / p.gpw;
    return MFM_OK;
}

/* [v1] the first-generation matrix kernel.  An LDS row (the D samples between two outputs) is 2*D plane bytes; the B
 * fragments are 16-byte reads, so rows are padded to 16-byte multiples when D is not a multiple of 8, and the taps (the A
 * operand) carry zeros over the padding: decimation 25 of etc/pocsag_rtlsdr.json = rows of 50 + 14 bytes, 128 taps = 5 full
 * rows + 3 taps = 326 elements -> 6 k-steps instead of 4.  Usable while at least 3/4 of a row is samples, the padded filter
 * fits the 16 k-steps of the streaming variant and every tap splits into two signed bytes.  62-output tiles (two 31-output
 * iterations) where they fit, else 31. */
void plan_v1(KernelPlan &p, uint32_t flags, const std::vector<Channel> &chans)
{
    const uint32_t T = p.T, D = p.D, C = p.C;
    const uint32_t row_bytes = shift_geometry(p, flags) ? 2u * D : (2u * D + 15u) & ~15u;
    const uint32_t k_elems = window_elems(T, D, row_bytes);
    if (!(8u * D >= 3u * row_bytes && k_elems <= 64u * MFM_MFMA_KQ_STREAM_MAX && !(flags & MFM_F_FORCE_DOT2))) {
        return;
    }
    for (const Channel &ch : chans) {
        for (uint32_t i = 0; i < T; i++) {
            if (ch.cre[i] > 32639 || ch.cim[i] > 32639 || ch.cim[i] < -32639) {
                return; /* 256*Wh + Wl with both in int8 needs W <= 32639 */
            }
        }
    }
    uint32_t kq = 1;
    while (64u * kq < k_elems) {
        kq *= 2;
    }
    p.m_kq_used = (k_elems + 63u) / 64u;
    const bool padded = row_bytes != 2u * D;
    const uint32_t rs_m = odd32_stride(row_bytes);
    /* samples a tile stages: its outputs' rows plus the rows the last window reaches into */
    auto nstage = [&](uint32_t ot) {
        return padded ? ((ot * D + ((64u * kq + row_bytes - 1u) / row_bytes) * D) + 3u) & ~3u : ((ot * D + 32u * kq) + 3u) & ~3u;
    };
    uint32_t ot = 0, plane = 0, lds = 0;
    const uint32_t want[] = { 2u * 31u, 31u }; /* new outputs per tile: two 31-output iterations, or one for large decimations */
    for (uint32_t cand : want) {
        const uint32_t nst = nstage(cand);
        const uint32_t rows = (nst + D - 1u) / D;
        const uint32_t pb = rows * rs_m;
        /* two staging buffers x two byte planes + atan LUT + staging offsets + rotator constants of up to 256 channels */
        const uint32_t nch_t = (nst / 4u + MFM_MFMA_NW * 64u - 1u) / (MFM_MFMA_NW * 64u); /* staging chunks per thread */
        const uint32_t need = 4u * pb + 2048u + nch_t * MFM_MFMA_NW * 64u * 4u + (kq > MFM_MFMA_KQ_MAX ? 2048u : 0u) +
                              (C <= 256u ? 32u * C : 0u);
        /* up to 80 KB two workgroups share a CU; beyond that one per CU is still far better than the v_dot2 kernel */
        /* the kernels are built for up to 4 chunks per thread with two iterations, up to MFM_M_CH_MAX with one
         * (and then only for 128-tap-class and longer filters) */
        const uint32_t nch_max = cand == 62u ? 4u : MFM_M_CH_MAX;
        if (cand == 31u && kq < MFM_MFMA_KQ_MAX) {
            continue;
        }
        if (need <= 150u * 1024u && nch_t <= nch_max) {
            ot = cand;
            plane = pb;
            lds = need;
            break;
        }
    }
    if (0 == ot) {
        return;
    }
    p.variant = 1;
    p.m_ks = kq;
    p.m_row_bytes = row_bytes;
    p.m_nstage = nstage(ot);
    p.m_ot = ot;
    p.m_rs = rs_m;
    p.m_plane_bytes = plane;
    p.m_lut_off = 4u * plane;
    p.m_lds_bytes = lds;
    /* planes at a fixed 16 KiB pitch when they fit and two workgroups still share a CU: the kernel then reaches the low-byte
     * plane and the second staging buffer through instruction immediates */
    if (plane <= MFM_M_PLANE_DIST && kq <= MFM_MFMA_KQ_MAX && ot == 62u) { /* streaming / single-iteration variants: packed planes */
        const uint32_t lds_fixed = 4u * MFM_M_PLANE_DIST + (lds - 4u * plane);
        if (2u * lds_fixed <= 160u * 1024u) {
            p.m_fixed_planes = true;
            p.m_lut_off = 4u * MFM_M_PLANE_DIST;
            p.m_lds_bytes = lds_fixed;
            lds = lds_fixed;
        }
    }
    p.m_nrb = (2u * C + 15u) / 16u;
    p.m_nslices = (p.m_nrb + MFM_MFMA_NW - 1u) / MFM_MFMA_NW;
    p.m_wg_per_cu = std::max(1u, std::min(2u, (160u * 1024u) / lds));
    p.m_ah_mask = tap_plane_mask(chans, T, D, row_bytes);
}

/* [sub] second generation, 64-output tiles, four sub-planes per byte plane (mfm_kernel.h): D % 32 == 0, <= 4 k-steps */
void plan_sub(KernelPlan &p, uint32_t flags)
{
    const uint32_t D = p.D;
    if (!(1u == p.variant && !(flags & MFM_F_FORCE_MFMA_V1) && p.m_ks <= 4u && (2u * D) % 64u == 0u)) {
        return;
    }
    const uint32_t kq = p.m_ks, row_bytes = 2u * D;
    const uint32_t rs_v = odd32_stride(row_bytes);
    const uint32_t extra = (64u * kq - 1u) / row_bytes; /* rows the last output's window reaches past the tile */
    const uint32_t rows = MFM_V3_LEAD + MFM_V3_OT + extra;
    const uint32_t sr = (rows + 3u) / 4u;
    uint32_t sp = sr * rs_v;
    sp = sp <= mfm_sp_pitch_v3() ? mfm_sp_pitch_v3() : (sp + 63u) & ~63u;
    const uint32_t nstage4 = rows * D / 4u; /* D % 16 == 0 here */
    const uint32_t nch = (nstage4 + 511u) / 512u;
    const uint32_t lds = 16u * sp + 2048u + nch * 512u * 4u + 1024u + 2048u; /* image, atan table, staging offsets, row constants + fold constants, exact-rotator table */
    if (nch > MFM_V3_CH_MAX || lds > 160u * 1024u) {
        return;
    }
    p.variant = 2;
    p.v_rs = rs_v;
    p.v_sp_pitch = sp;
    p.v_nstage4 = nstage4;
    p.v_lds_bytes = lds;
    p.v_wg_per_cu = std::max(1u, std::min(2u, (160u * 1024u) / lds));
#ifdef MFM_EXP_ONE_WG_PER_CU /* occupancy experiment (tools/exp/snapeng.sh): LDS padded so that one workgroup fits a CU */
    p.v_lds_bytes = 100u * 1024u;
    p.v_wg_per_cu = 1u;
#endif
    for (uint32_t k = 0; k < 4; k++) {
        p.v_cross[k] = k < kq ? (64u * k) / row_bytes : 0u;
        p.v_within[k] = k < kq ? (64u * k) % row_bytes : 0u;
    }
}

/* [crow] decimations that are multiples of 8 but not of 32 (40: etc/multifm.json, etc/multifm_1ch.json), <= 4 k-steps: the
 * chunk-row layout (mfm_kernel.h).  t_per = chunks of four outputs; slots: one per four staged rows, plus the window's reach */
void plan_crow(KernelPlan &p, uint32_t flags)
{
    const uint32_t D = p.D;
    if (!(1u == p.variant && !(flags & MFM_F_FORCE_MFMA_V1) && p.m_ks <= 4u && D % 8u == 0u && (2u * D) % 64u != 0u)) {
        return;
    }
    const uint32_t kq = p.m_ks, row_bytes = 2u * D, cpo = D / 8u, per = 4u * cpo;
    const uint32_t extra = (64u * kq - 1u) / row_bytes;
    const uint32_t rows = MFM_V3_LEAD + MFM_V3_OT + extra;
    const uint32_t nchunks16 = (rows * row_bytes + 15u) / 16u;
    const uint32_t x_max = cpo * 3u + 4u * (kq - 1u);
    const uint32_t pitch = std::max((nchunks16 + per - 1u) / per + 1u, 16u + 1u + x_max / per + 1u);
    const uint32_t plane = ((per + 3u) * pitch * 16u + 63u) & ~63u;
    const uint32_t nstage4 = rows * D / 4u; /* D % 8 == 0 */
    const uint32_t nch = (nstage4 + 511u) / 512u;
    const uint32_t lds = 4u * plane + 2048u + nch * 512u * 4u + 1024u + 2048u + nch * 512u * 4u;
    if (nch > MFM_V3_CH_MAX || lds > 160u * 1024u) {
        return;
    }
    p.variant = 2;
    p.v_layout = 1;
    p.v_t_per = per;
    p.v_t_pitch = pitch;
    p.v_sp_pitch = plane / 4u; /* plane pitch = 4 * sp_pitch, buffer pitch = 8 * sp_pitch, as in the sub-plane layout */
    p.v_nstage4 = nstage4;
    p.v_lds_bytes = lds;
    p.v_wg_per_cu = std::max(1u, std::min(2u, (160u * 1024u) / lds));
}

/* [pad25] decimation 25 (etc/pocsag_rtlsdr.json), <= 150 taps: rows of 50 plane bytes padded to 64, so that a k-step is
 * exactly one row and a window spans six of them (layout 2, mfm_kernel.h); sub-planes at the fixed pitch, the image staged
 * sample by sample.  The tap fragments are laid out for six k-steps. */
void plan_pad25(KernelPlan &p, uint32_t flags)
{
    if (!(p.variant >= 1u && !(flags & MFM_F_FORCE_MFMA_V1) && 25u == p.D && p.T <= 150u)) {
        return;
    }
    p.variant = 2;
    p.v_layout = 2;
    p.v_rs = 96u;
    p.v_sp_pitch = mfm_sp_pitch_v3();
    p.v_nstage4 = (73u * 25u + 3u + 3u) / 4u; /* 16-byte chunks covering the image wherever it starts inside the first one */
    p.v_lds_bytes = 16u * mfm_sp_pitch_v3() + 2048u + 4u * 512u * 4u + 1024u + 2048u;
    p.v_wg_per_cu = 2u;
    for (uint32_t k = 0; k < 4; k++) {
        p.v_cross[k] = k;
        p.v_within[k] = 0;
    }
    p.m_ks = 6u;
    p.m_kq_used = 6u;
}

/* [shift] decimations 1, 2, 4 on the long-filter kernel's shifted copies (mfm_kernel_v3l.hip, SHIFT): whole-tile images of
 * 8 / D copies, one row block per wave; the first generation's geometry does not apply to rows this short, so where no
 * instance is built the v_dot2 kernel runs */
void plan_shift(KernelPlan &p, uint32_t flags)
{
    if (!(shift_geometry(p, flags) && p.variant >= 1u)) {
        return;
    }
    const uint32_t T = p.T, D = p.D;
    const uint32_t kq_inst = p.m_kq_used <= 4u ? 4u : p.m_kq_used <= 8u ? 8u : 16u;
    const uint32_t nc = 8u / D;
    const uint32_t img_samples = 63u * D + T;                       /* what the tile's 64 windows cover */
    const uint32_t read_bytes = 2u * D * 63u + 64u * kq_inst + 16u; /* ... and what the instance's fragment reads touch */
    /* bytes between two copies: at least the copy, and 2 D (mod 16) sixteen-byte units - the sixteen columns of a fragment read
     * (copy n % nc, offset 16 (n / nc)) then fall into sixteen different groups of four LDS banks */
    uint32_t cp16 = (std::max(2u * img_samples, read_bytes) + 15u) / 16u;
    while (cp16 % 16u != (2u * D) % 16u) {
        cp16++;
    }
    const uint32_t plane = nc * cp16 * 16u;
    const uint32_t aux = 8u * 8u * MFM_V3L_TP * 4u + 512u + 2048u;
    const uint32_t lds = 4u * plane + 2048u + 2048u + aux;
    mfm_launch_v3 probe{};
    probe.layout = 3u;
    probe.shift = 1u;
    probe.kq = kq_inst;
    probe.kq_used = p.m_kq_used;
    probe.nh = (uint32_t)__builtin_popcount(p.m_ah_mask);
    probe.ng = 4u;
    probe.rb = 1u;
    probe.nstage4 = img_samples;
    const void *fn = nullptr;
    if (!(img_samples <= 4u * 512u && lds <= 160u * 1024u && mfm_select_channel_kernel_v3(&probe, 0, &fn) == hipSuccess)) {
        p.variant = 0; /* the v_dot2 kernel */
        return;
    }
    p.variant = 2;
    p.v_layout = 3u;
    p.v_shift = 1u;
    p.v_copy_pitch = cp16 * 16u;
    p.v_rs = 2u * D;
    p.v_plane = plane;
    p.v_sp_pitch = 0;
    p.v_ng = 4u;
    p.v_rb = 1u;
    p.v_nstage4 = img_samples;
    p.v_nstage_p = T;
    p.v_sta_bytes = 2048u;
    p.v_lds_bytes = lds;
    p.v_wg_per_cu = 1u; /* (per input format: mfm_v3l_wg_per_cu) */
    p.v_kq = kq_inst;
    p.v_nh = probe.nh;
    kstep_order(p.m_ah_mask, p.m_kq_used, kq_inst, p.v_kperm);
}

/* Layout 3 (mfm_kernel_v3l.hip): the first generation's image - plain rows of m_row_bytes plane bytes at stride m_rs, any
 * decimation - holding a whole 64-output tile, or a part of one; same tap fragments, same row constants.  Two row blocks per
 * wave (slices of 128 channels) share every B fragment and every staged image: half the LDS traffic and half the staging work
 * per (channel, output), for two waves per SIMD instead of four.  The first (row blocks per wave, column groups per image)
 * candidate that fits and is built wins. */
struct l3_cand {
    uint32_t rb, ng;
};
bool plan_layout3(KernelPlan &p, uint32_t flags, const l3_cand *cand, size_t nr_cand)
{
    const uint32_t D = p.D, row_bytes = p.m_row_bytes, rs_l = p.m_rs;
    const uint32_t kq_inst = mfm_v3l_built_kq(p.m_kq_used);
    const uint32_t nh = (uint32_t)__builtin_popcount(p.m_ah_mask);
    const uint32_t k_elems = window_elems(p.T, D, row_bytes);
    const uint32_t reach = (k_elems - 1u) / row_bytes;                 /* rows the last window reaches past its own */
    const uint32_t reach_read = (64u * kq_inst - 1u) / row_bytes + 1u; /* ... and what the instance's fragment reads touch */
    const uint32_t nh_inst = mfm_v3l_built_nh(kq_inst, nh);
    for (size_t ci = 0; ci < nr_cand; ci++) {
        const uint32_t ng = cand[ci].ng, rbw = cand[ci].rb;
        /* two row blocks: more than 64 channels, and two row blocks' taps fit 128 registers */
        if (2u == rbw && (p.m_nrb <= 8u || 8u * (kq_inst + nh_inst) > 128u || (flags & MFM_F_V3L_ONE_ROW_BLOCK))) {
            continue;
        }
        const uint32_t opi = 16u * ng;
        const uint32_t plane_used = (opi + std::max(reach, reach_read)) * rs_l;
        const uint32_t plane = mfm_v3l_plane_pitch(rbw); /* a constant: the low plane's reads are "high plane + immediate" */
        const uint32_t nstage4 = ((opi + reach) * D + 3u) / 4u;
        const uint32_t nch = (nstage4 + 511u) / 512u;
        if (nch > MFM_V3_CH_MAX || plane_used > plane || kq_inst > p.m_ks) {
            continue;
        }
        /* the instance's count of chunks (a surplus chunk is loaded and not stored); 16-bit offsets where no chunk straddles rows */
        const uint32_t sta = mfm_v3l_built_nch(nch) * ((D % 4u) != 0u ? 1536u : 1024u); /* 16-bit offsets (+ a byte per chunk: rows split) */
        const uint32_t aux = 8u * 8u * rbw * MFM_V3L_TP * 4u + 512u * rbw + 2048u * rbw;
        const uint32_t lds = 4u * plane + 2048u + sta + aux;
        if (lds > 160u * 1024u) {
            continue;
        }
        /* is the int16 instance for this geometry built?  (All are but a few that would need more than 256 registers.)  It
         * must be known HERE: the second generation orders its rows by rotator class, the first does not. */
        mfm_launch_v3 probe{};
        probe.layout = 3u;
        probe.kq = kq_inst;
        probe.kq_used = p.m_kq_used;
        probe.nh = nh;
        probe.ng = ng;
        probe.rb = rbw;
        probe.nstage4 = nstage4;
        probe.split_rows = (D % 4u) != 0u ? 1u : 0u; /* (sample-by-sample staging: instances of their own, one row block per wave) */
        probe.ah_mask = p.m_ah_mask;
        const void *fn = nullptr;
        if (mfm_select_channel_kernel_v3(&probe, 0, &fn) != hipSuccess) {
            continue;
        }
        p.variant = 2;
        p.v_rb = rbw;
        p.v_layout = 3u;
        p.v_rs = rs_l;
        p.v_plane = plane;
        p.v_sp_pitch = 0;
        p.v_ng = ng;
        p.v_nstage4 = nstage4;
        p.v_nstage_p = ((1u + reach) * D + 3u) / 4u;
        p.v_sta_bytes = sta;
        p.v_lds_bytes = lds;
        p.v_wg_per_cu = 1u; /* two waves per SIMD hold a long filter's taps: one workgroup per CU */
        p.v_kq = kq_inst;
        p.v_nh = nh;
        kstep_order(p.m_ah_mask, p.m_kq_used, kq_inst, p.v_kperm);
        return true;
    }
    return false;
}

/* [v3l] filters of 129..512 taps (8..16 k-steps) on layout 3: slices of 128 channels on quarter-tile images where there are
 * more than 64 channels and two row blocks' taps fit 128 registers; else slices of 64 on whole- or half-tile images (decimation
 * 400 of configs[4]: 112 KB per whole-tile image of both planes) */
void plan_v3l(KernelPlan &p, uint32_t flags)
{
    if (1u == p.variant && !(flags & (MFM_F_FORCE_MFMA_V1 | MFM_F_STREAM_TAPS)) && p.m_ks >= 8u && p.m_ks <= MFM_V3L_KQ_MAX) {
        const l3_cand cand[3] = { { 2u, 1u }, { 1u, 4u }, { 1u, 2u } };
        plan_layout3(p, flags, cand, 3);
    }
}

/* [s128] 128-tap filters of the [sub] geometry on SLICES OF 128 CHANNELS where there are that many (multifm/receiver.c:195-244
 * builds as many channels as the configuration lists; north_star's shape is 1024 of them on one GPU): layout 3 with two row
 * blocks per wave on whole-tile images.  The sub-plane layout stays what runs when the instance is not built. */
void plan_s128(KernelPlan &p, uint32_t flags)
{
    if (2u == p.variant && 0u == p.v_layout && 4u == p.m_ks && (2u * p.D) % 64u == 0u &&
        !(flags & (MFM_F_FORCE_MFMA_V1 | MFM_F_SLICE_64)) && ((flags & MFM_F_SLICE_128) || p.C >= kSlice128MinChannels)) {
        const l3_cand cand[1] = { { 2u, 4u } };
        plan_layout3(p, flags, cand, 1);
    }
}

/* ---- rotator classes (filter/direct_fir.c:151-172,406-413).  An increment of exactly (16384, 0) - every channel whose offset
 *      is a multiple of the output rate, e.g. a 25 kHz grid at 2.4 MS/s / 96 - leaves the rotator at (16384, 0) for ever, and
 *      r14(f * 16384) = f: nothing to do.  An increment of (-16384, 0) - offsets at odd multiples of half the output rate - makes
 *      it alternate between (16384, 0) and (-16384, 0), and r14(f * -16384) = -f with the int16 cast's wrap: one packed
 *      multiply by +-1.  An increment of (0, +-16384) - offsets at odd multiples of a quarter of the output rate - walks the
 *      four axis points: r14(f * rot) = f * j^m, a swap of the halves and two signs.  Everything else is the general case (two
 *      Q14 dot products against the tabulated rotator and a second rounding). ---- */
uint32_t chan_class(const Channel &ch)
{
    if ((ch.incr_re == 16384 && ch.incr_im == 0) || (ch.incr_re == 0 && ch.incr_im == 0)) {
        return MFM_RC_IDENT; /* direct_fir.c:406 skips the derotation altogether for a zero increment */
    }
    if (ch.incr_re == -16384 && ch.incr_im == 0) {
        return MFM_RC_FLIP;
    }
    return (ch.incr_re == 0 && (ch.incr_im == 16384 || ch.incr_im == -16384)) ? MFM_RC_QUARTER : MFM_RC_GENERAL;
}

/* quarter turns per output: rot after k outputs = j^(turns * k) * 16384 for the exact classes */
uint32_t chan_turns(const Channel &ch)
{
    return ch.incr_im == 16384 ? 1u : ch.incr_im == -16384 ? 3u : ch.incr_re == -16384 ? 2u : 0u;
}

/* The second-generation kernel runs a 64-channel slice without the table loads and the derotation arithmetic when all its
 * channels are exact, so its rows are ordered by class (stable); where a row's PCM goes is in its mfm_chan_info. */
void plan_rows(KernelPlan &p, const std::vector<Channel> &chans)
{
    const uint32_t C = p.C;
    const bool v3 = 2u == p.variant;
    p.perm.resize(C);
    for (uint32_t c = 0; c < C; c++) {
        p.perm[c] = c;
    }
    if (v3) {
        std::stable_sort(p.perm.begin(), p.perm.end(),
                         [&](uint32_t a, uint32_t b) { return chan_class(chans[a]) > chan_class(chans[b]); });
    }
    for (uint32_t c = 0; c < C; c++) {
        p.rot_exact_channels += chan_class(chans[c]) != MFM_RC_GENERAL ? 1u : 0u;
    }
    p.v_rc = MFM_RC_IDENT;
    for (uint32_t sl = 0; sl < p.m_nslices && v3; sl++) {
        uint32_t cls = MFM_RC_IDENT; /* rows past the last channel have zero taps and store nothing */
        for (uint32_t c = sl * 64u; c < std::min(C, sl * 64u + 64u); c++) {
            cls = std::min(cls, chan_class(chans[p.perm[c]]));
        }
        p.v_rc = std::min(p.v_rc, cls);
        p.rot_fast_slices += cls != MFM_RC_GENERAL ? 1u : 0u;
    }
    if (!v3 || p.any_iq || p.v_layout >= 2u) {
        p.v_rc = MFM_RC_GENERAL; /* the exact-rotator instances are built without the filtered-IQ output, and for the
                                    sub-plane / chunk-row geometries only */
    }
}

/* the geometry half of a second-generation launch description for blocks of input format fmt */
void fill_v3(const KernelPlan &p, uint32_t flags, int fmt, mfm_launch_v3 &V)
{
    V.decim = p.D;
    V.x_last4 = p.v_shift ? p.cap_in - 1u : (p.cap_in - 4u) & ~3u;
    V.kq = p.m_ks;
    V.rs = p.v_rs;
    V.sp_pitch = p.v_sp_pitch;
    V.plane_pitch = 4u * p.v_sp_pitch;
    V.buf_pitch = 8u * p.v_sp_pitch;
    V.nstage4 = p.v_nstage4;
    V.lut_off = 16u * p.v_sp_pitch;
    V.sta_off = V.lut_off + 2048u;
    for (int k = 0; k < 4; k++) {
        V.cross[k] = p.v_cross[k];
        V.within[k] = p.v_within[k];
    }
    V.layout = p.v_layout;
    V.t_per = p.v_t_per;
    V.t_pitch = p.v_t_pitch;
    if (3u == p.v_layout) {
        /* long filters: [two buffers of two byte planes | atan table | staging offsets | transposition areas + per-wave constants] */
        V.plane_pitch = p.v_plane;
        V.buf_pitch = 2u * p.v_plane;
        V.lut_off = 4u * p.v_plane;
        V.sta_off = V.lut_off + 2048u;
        V.tp_off = V.sta_off + p.v_sta_bytes;
        V.row_bytes = p.m_row_bytes;
        V.split_rows = (p.D % 4u) != 0u ? 1u : 0u;
        V.kq = p.v_kq;
        V.kq_used = p.m_kq_used;
        V.nh = p.v_nh;
        for (int k = 0; k < 4; k++) {
            V.kperm[k] = p.v_kperm[k];
        }
        V.ng = p.v_ng;
        V.rb = p.v_rb;
        V.nstage_p = p.v_nstage_p;
        V.shift = p.v_shift;
        if (p.v_shift) {
            V.sp_pitch = p.v_copy_pitch;
        }
    }
    V.nslices = p.v_nslices;
    V.nrb = p.m_nrb;
    V.nchan = p.C;
    V.pcm_scope = (p.C >= kPcmWriteThroughMinChannels && !(flags & MFM_F_PCM_WRITE_BACK)) ? 1u : 0u;
    V.out_stride = p.out_stride;
    V.ah_mask = p.m_ah_mask;
    V.rc = p.v_rc;
    if (fmt != MFM_IN_CS16) {
        /* the buffer holds 2-byte samples: twice as many fit, a 16-byte chunk is 8 of them */
        V.in8 = fmt == MFM_IN_RTLSDR_U8 ? 7u : 14u;
        V.in8_xor = fmt == MFM_IN_RTLSDR_U8 ? 0x80808080u : 0u;
        V.nstage4 = 2u == p.v_layout ? (73u * 25u + 7u + 7u) / 8u : p.v_nstage4 / 2u;
        V.x_last4 = (2u * p.cap_in - 8u) & ~7u;
        if (3u == p.v_layout) {
            /* a staging chunk stays 4 samples there - an 8-byte load */
            V.nstage4 = p.v_nstage4;
            V.x_last4 = (2u * p.cap_in - 4u) & ~3u;
            if (p.v_shift) {
                V.x_last4 = 2u * p.cap_in - 1u; /* one-sample loads */
            }
        }
    }
}

/* ... of a first-generation one */
void fill_mfma(const KernelPlan &p, uint32_t flags, int fmt, mfm_launch_mfma &M)
{
    M.decim = p.D;
    M.x_last4 = (p.cap_in - 4u) & ~3u;
    M.kq = p.m_ks;
    M.kq_used = p.m_kq_used;
    M.ot = p.m_ot;
    M.nstage = p.m_nstage;
    M.rs = p.m_rs;
    M.row_bytes = p.m_row_bytes;
    M.split_rows = (p.D % 4u) != 0u ? 1u : 0u;
    M.plane_bytes = p.m_plane_bytes;
    M.fixed_planes = p.m_fixed_planes ? 1u : 0u;
    M.lut_off = p.m_lut_off;
    M.sta_off = p.m_lut_off + 2048u;
    M.bof_off = M.sta_off + ((M.nstage / 4u + MFM_MFMA_NW * 64u - 1u) / (MFM_MFMA_NW * 64u)) * MFM_MFMA_NW * 64u * 4u;
    M.tbl_off = p.C <= 256u ? M.bof_off + (p.m_ks > MFM_MFMA_KQ_MAX ? 2048u : 0u) : 0u;
    M.nslices = p.m_nslices;
    M.nrb = p.m_nrb;
    M.nchan = p.C;
    M.out_stride = p.out_stride;
    M.ah_mask = p.m_ah_mask;
    M.stream_taps = (flags & MFM_F_STREAM_TAPS) ? 1u : 0u;
    if (fmt != MFM_IN_CS16) {
        /* the buffer holds 2-byte samples: twice as many fit; a staging chunk (4 samples) is an 8-byte load */
        M.in8 = fmt == MFM_IN_RTLSDR_U8 ? 7u : 14u;
        M.in8_xor = fmt == MFM_IN_RTLSDR_U8 ? 0x80808080u : 0u;
        M.x_last4 = (2u * p.cap_in - 4u) & ~3u;
    }
}

/* ... of a v_dot2 one */
void fill_dot2(const KernelPlan &p, mfm_launch &L)
{
    L.decim = p.D;
    L.nchunks = p.nchunks;
    L.nstage = (64u * p.opl - 1) * p.D + p.T;
    L.rs2 = p.rs2;
    L.lut_off = p.lut_off;
    L.ngroups = p.ngroups;
    L.gpw = p.gpw;
    L.nslices = p.nslices;
    L.nchan = p.C;
    L.out_stride = p.out_stride;
}

/* which instance runs blocks of each input format, and the launch description it is given */
int plan_formats(KernelPlan &p, uint32_t flags)
{
    const int dbg_iq = p.any_iq ? 1 : 0;
    for (int fmt = MFM_IN_CS16; fmt <= MFM_IN_RTLSDR_U8; fmt++) {
        FormatPlan &f = p.fmt[fmt];
        if (fmt != MFM_IN_CS16 && !p.raw8_ok) {
            continue;
        }
        hipError_t err;
        if (2u == p.variant) {
            fill_v3(p, flags, fmt, f.V);
            err = mfm_select_channel_kernel_v3(&f.V, dbg_iq, &f.kfn);
            f.lds_bytes = p.v_lds_bytes;
            /* (the long-filter kernel's small 8-bit instances are built for two workgroups per CU, the others for one) */
            f.wg_per_cu = (3u == p.v_layout && 2u * p.v_lds_bytes <= 160u * 1024u) ? mfm_v3l_wg_per_cu(&f.V) : p.v_wg_per_cu;
            f.taps_resident = 3u == p.v_layout;
        } else if (1u == p.variant) {
            fill_mfma(p, flags, fmt, f.M);
            uint32_t wps = 4;
            err = mfm_select_channel_kernel_mfma(&f.M, dbg_iq, &f.kfn, &wps);
            f.lds_bytes = p.m_lds_bytes;
            /* a resident long-filter instance takes a SIMD's registers with two waves: one workgroup per CU */
            f.taps_resident = wps < 4u;
            f.wg_per_cu = f.taps_resident ? 1u : p.m_wg_per_cu;
        } else {
            fill_dot2(p, f.L);
            err = mfm_select_channel_kernel(p.opl, dbg_iq, &f.kfn);
            f.lds_bytes = p.lds_bytes;
        }
        if (err != hipSuccess) {
            return fail(MFM_E_DEVICE, "no variant-%u kernel instance for input format %d (error %d)", p.variant, fmt, (int)err);
        }
    }
    return MFM_OK;
}

} /* namespace */

/* The selection reads in the order of the rule tags of tests/test_kernel_forms.py: each planner after the first two may
 * replace what the ones before it chose. */
int plan_channel_kernel(const mfm_engine_config &cfg, const std::vector<Channel> &chans, uint32_t nr_taps, KernelPlan &p)
{
    if (chans.empty()) {
        return fail(MFM_E_INVAL, "no channels");
    }
    p = KernelPlan();
    p.T = nr_taps;
    p.D = cfg.decimation;
    p.C = (uint32_t)chans.size();
    const uint32_t flags = cfg.flags;
    int rc = plan_dot2(p);
    if (rc != MFM_OK) {
        return rc;
    }
    p.cap_in = (uint32_t)input_capacity(cfg.max_block_samples, cfg.coalesce_samples, p.T);
    /* a multiple of 8 outputs: channel rows of the PCM buffer start 16-byte aligned (8-byte PCM / 16-byte IQ stores) */
    p.out_stride = ((p.cap_in - p.T) / p.D + 1 + 7) & ~7u;
    for (const Channel &c : chans) {
        p.any_iq |= c.want_iq;
    }
    /* the kernels address outputs with 32-bit byte offsets from the buffer base: 2 bytes per PCM sample, 4 per
     * filtered-IQ sample, plus the dump slots behind the last row */
    const uint64_t out_limit = p.any_iq ? (1ull << 30) : (1ull << 31);
    if ((uint64_t)p.C * p.out_stride + 64 >= out_limit) {
        return fail(MFM_E_INVAL, "channels x outputs per block = %llu exceeds %llu (use smaller blocks)",
                    (unsigned long long)p.C * p.out_stride, (unsigned long long)out_limit);
    }

    plan_v1(p, flags, chans);
    plan_sub(p, flags);
    plan_crow(p, flags);
    plan_pad25(p, flags);
    plan_shift(p, flags);
    plan_v3l(p, flags);
    plan_s128(p, flags);

    p.v_nslices = (2u == p.variant && 3u == p.v_layout) ? (p.m_nrb + 8u * p.v_rb - 1u) / (8u * p.v_rb) : p.m_nslices;
    plan_rows(p, chans);
    /* 8-bit input read as it is: both matrix kernels have the form for it (not built for the filtered-IQ debug output) */
    p.raw8_ok = p.variant >= 1u && (2u != p.variant || (p.v_nstage4 / 2u + 511u) / 512u <= 4u) && !p.any_iq &&
                !(flags & MFM_F_WIDEN_8BIT);
    return plan_formats(p, flags);
}

void plan_form_stats(const KernelPlan &p, mfm_stats *st)
{
    const bool mfma = p.variant >= 1u;
    st->kernel_variant = p.variant;
    st->rot_exact_channels = p.rot_exact_channels;
    st->rot_fast_slices = p.rot_fast_slices;
    st->k_steps = mfma ? p.m_ks : 0u;
    st->tap_hi_mask = mfma ? p.m_ah_mask : 0u;
    st->taps_resident = p.fmt[MFM_IN_CS16].taps_resident ? 1u : 0u;
    st->slice_channels = 2u == p.variant ? ((3u == p.v_layout) ? 64u * p.v_rb : 64u) : mfma ? 64u : 0u;
    st->outputs_per_tile = 2u == p.variant ? MFM_V3_OT : mfma ? p.m_ot : 64u * p.opl;
    st->lds_bytes = p.fmt[MFM_IN_CS16].lds_bytes;
}

/* ---- host tables ---- */

namespace {

inline void rot_step(int16_t &rr, int16_t &ri, int16_t ir, int16_t ii)
{
    /* filter/direct_fir.c:166-167 -> filter/complex.h:51-62 */
    const int32_t a = rr, b = ri;
    const int16_t nr = (int16_t)mfm_r14_wide(a * ir - b * ii);
    const int16_t ni = (int16_t)mfm_r14_wide(a * ii + b * ir);
    rr = nr;
    ri = ni;
}

/* Brent's cycle finder on the rotator recurrence started at (16384, 0) (direct_fir.c:78-79). */
bool rot_cycle(int16_t ir, int16_t ii, uint64_t limit, uint32_t *mu_out, uint32_t *lam_out)
{
    int16_t tr = 16384, ti = 0, hr = 16384, hi = 0;
    uint64_t power = 1, lam = 1;
    rot_step(hr, hi, ir, ii);
    while (!(tr == hr && ti == hi)) {
        if (power == lam) {
            tr = hr;
            ti = hi;
            power *= 2;
            lam = 0;
        }
        rot_step(hr, hi, ir, ii);
        lam++;
        if (lam > limit) {
            return false;
        }
    }
    tr = 16384, ti = 0, hr = 16384, hi = 0;
    for (uint64_t i = 0; i < lam; i++) {
        rot_step(hr, hi, ir, ii);
    }
    uint64_t mu = 0;
    while (!(tr == hr && ti == hi)) {
        rot_step(tr, ti, ir, ii);
        rot_step(hr, hi, ir, ii);
        mu++;
        if (mu > limit) {
            return false;
        }
    }
    *mu_out = (uint32_t)mu;
    *lam_out = (uint32_t)lam;
    return true;
}

/* tap table of the v_dot2 kernel: [group][chunk][tap in chunk][channel in group]{(cr,-ci),(ci,cr)}, and the LDS byte offset
 * of each tap */
void build_dot2_taps(const KernelPlan &p, const std::vector<Channel> &chans, HostTables &t)
{
    const uint32_t T = p.T, D = p.D;
    t.coef.assign((size_t)p.ngroups * p.nchunks * MFM_TG * MFM_CG * 2, 0u);
    for (uint32_t c = 0; c < p.C; c++) {
        const Channel &ch = chans[c];
        const uint32_t g = c / MFM_CG, cc = c % MFM_CG;
        for (uint32_t i = 0; i < T; i++) {
            const uint32_t chunk = i / MFM_TG, k = i % MFM_TG;
            const size_t at = ((((size_t)g * p.nchunks + chunk) * MFM_TG + k) * MFM_CG + cc) * 2;
            const int32_t cr = ch.cre[i], ci = ch.cim[i];
            t.coef[at + 0] = mfm_pack16(cr, -ci);
            t.coef[at + 1] = mfm_pack16(ci, cr);
        }
    }
    t.tapoff.assign((size_t)p.nchunks * MFM_TG, 0u);
    for (uint32_t i = 0; i < T; i++) {
        t.tapoff[i] = ((i % D) * p.rs2 + i / D) * 4u;
    }
}

/* the matrix kernels' A fragments, m_ks k-steps per row block in plan.perm's row order, and row constants */
void build_fragments(const KernelPlan &p, const std::vector<Channel> &chans, HostTables &t)
{
    const uint32_t T = p.T, D = p.D, C = p.C, kq = p.m_ks, row_bytes = p.m_row_bytes;
    /* W[2c] = (cr0,-ci0,cr1,-ci1..), W[2c+1] = (ci0,cr0,ci1,cr1..) (filter/complex.h:40-46) */
    const uint32_t K = 64u * kq;
    auto w_at = [&](uint32_t row, uint32_t k) -> int32_t {
        /* element k of a window = byte k % row_bytes of LDS row k / row_bytes: sample (k / row_bytes) * D +
         * (k % row_bytes) / 2 while the byte is inside the 2 * D sample bytes, padding (zero tap) behind them */
        const uint32_t c = row / 2u, pos = k % row_bytes, i = (k / row_bytes) * D + pos / 2u;
        if (c >= C || pos >= 2u * D || i >= T) {
            return 0;
        }
        const int32_t cr = chans[p.perm[c]].cre[i], ci = chans[p.perm[c]].cim[i];
        if (row & 1u) {
            return (k & 1u) ? cr : ci;
        }
        return (k & 1u) ? -ci : cr;
    };
    /* v_mfma_i32_16x16x64_i8 A operand: lane (kg = lane >> 4, i = lane & 15) holds row i, elements 64*kq + 16*kg + j,
     * j = 0..15 */
    t.afrag.assign((size_t)p.m_nrb * kq * 2 * 64 * 4, 0u);
    t.krow.assign((size_t)p.m_nrb * 16, 0);
    uint8_t *ab = reinterpret_cast<uint8_t *>(t.afrag.data());
    for (uint32_t rb = 0; rb < p.m_nrb; rb++) {
        for (uint32_t i = 0; i < 16; i++) {
            const uint32_t row = rb * 16u + i;
            uint32_t sum = 0;
            for (uint32_t k = 0; k < K; k++) {
                const int32_t w = w_at(row, k);
                sum += (uint32_t)w;
                const int32_t wl = (int8_t)(w & 0xff);
                const int32_t wh = (w - wl) >> 8;
                const uint32_t kst = k / 64u, gg = (k % 64u) / 16u, j = k % 16u;
                const uint32_t ln = gg * 16u + i;
                const size_t base = ((((size_t)rb * kq + kst) * 2u) * 64u + ln) * 16u + j;
                ab[base] = (uint8_t)(int8_t)wh;             /* plane 0: high bytes */
                ab[base + 64u * 16u] = (uint8_t)(int8_t)wl; /* plane 1: low bytes */
            }
            /* El = (e & 255) - 128 puts 128 * sum(W) into every product sum; 8192 is the rounding bias of the first
             * round_q30_q15 (filter/complex.h:30-34), added here once */
            t.krow[(size_t)rb * 16 + i] = (int32_t)(128u * sum + 8192u);
        }
    }
    if (2u == p.variant && 3u == p.v_layout) {
        /* the long-filter kernel's fragments: v_kq k-steps per row block, in the order v_kperm */
        const size_t step_dw = 2u * 64u * 4u; /* dwords of one k-step: two planes x 64 lanes x 16 bytes */
        std::vector<uint32_t> af3((size_t)p.m_nrb * p.v_kq * step_dw, 0u);
        for (uint32_t rb = 0; rb < p.m_nrb; rb++) {
            for (uint32_t j = 0; j < p.v_kq; j++) {
                const uint32_t src = (p.v_kperm[j >> 2] >> (8u * (j & 3u))) & 0xffu;
                if (src < p.m_ks) { /* (a step past the laid-out ones holds zero taps) */
                    memcpy(&af3[((size_t)rb * p.v_kq + j) * step_dw], &t.afrag[((size_t)rb * p.m_ks + src) * step_dw], step_dw * 4u);
                }
            }
        }
        t.afrag.swap(af3);
    }
    if (p.raw8_ok) {
        /* 8-bit input read as it is (mfm_kernel_v3.hip, IN8): x = alpha * s + beta with s the byte as int8, so the row
         * constant is (beta * sum(W) + 8192) / alpha - exact for all three forms.  krow = 128 * sum(W) + 8192. */
        for (int fmt = MFM_IN_CS8; fmt <= MFM_IN_RTLSDR_U8; fmt++) {
            std::vector<int32_t> &k8 = t.krow8[fmt];
            k8.resize(t.krow.size());
            for (size_t i = 0; i < t.krow.size(); i++) {
                const uint32_t sum = (uint32_t)(((int64_t)t.krow[i] - 8192) / 128); /* |sum(W)| < 2^24: no wrap in krow */
                k8[i] = fmt == MFM_IN_RTLSDR_U8 ? (int32_t)(sum + 64u)        /* (128 * sum + 8192) / 128 */
                        : fmt == MFM_IN_CU8     ? (int32_t)(8192u - 127u * sum) /* beta = -127 */
                                                : 8192;                          /* cs8: beta = 0 */
            }
        }
    }
}

/* rotator tables, one per distinct increment */
int build_rotators(const KernelPlan &p, std::vector<Channel> &chans, HostTables &t)
{
    std::map<std::pair<int16_t, int16_t>, std::pair<uint64_t, std::pair<uint32_t, uint32_t>>> seen;
    std::vector<uint2> &rot = t.rot;
    for (Channel &ch : chans) {
        const auto key = std::make_pair(ch.incr_re, ch.incr_im);
        auto it = seen.find(key);
        if (it == seen.end()) {
            uint32_t mu = 0, lam = 1;
            int16_t ir = ch.incr_re, ii = ch.incr_im;
            if (0 == ir && 0 == ii) {
                /* direct_fir.c:406 skips derotation for a zero increment; a constant (16384,0) rotator is the identity
                 * through both Q14 roundings */
                ir = 16384;
                ii = 0;
            }
            if (!rot_cycle(ir, ii, kMaxRotEntries, &mu, &lam)) {
                return fail(MFM_E_INVAL, "rotator (%d,%d) has no cycle within %llu steps", ir, ii, (unsigned long long)kMaxRotEntries);
            }
            /* unroll short cycles to at least one tile's worth of entries: a multiple of a period is a period, and the
             * kernels then fold an index with one conditional subtraction */
            lam = lam * ((kMaxOutputsPerTile + lam - 1) / lam);
            const uint64_t n = (uint64_t)mu + lam + kMaxOutputsPerTile;
            const uint64_t base = rot.size() + 1; /* one dummy entry in front: index -1 is readable */
            rot.resize(rot.size() + 1 + n);
            rot[base - 1] = make_uint2(0, 0);
            int16_t rr = 16384, ri = 0;
            for (uint64_t k = 0; k < n; k++) {
                if (ri == INT16_MIN) {
                    return fail(MFM_E_INVAL, "rotator state reached -32768");
                }
                rot[base + k] = make_uint2(mfm_pack16(rr, -(int32_t)ri), mfm_pack16(ri, rr));
                rot_step(rr, ri, ir, ii);
            }
            it = seen.emplace(key, std::make_pair(base, std::make_pair(mu, lam))).first;
        }
        ch.rot_base = it->second.first;
        ch.mu = it->second.second.first;
        ch.lam = it->second.second.second;
    }
    if (rot.size() >= (1ull << 29)) {
        return fail(MFM_E_INVAL, "rotator tables need %zu entries (limit 2^29: byte offsets are 32-bit)", rot.size());
    }
    if (2u == p.variant && mfm_rot_entry_bytes_v3() == 4u) {
        /* the second-generation kernel's build takes 4-byte entries (rr | ri << 16): half the table bytes per output */
        t.rot4.resize(rot.size());
        for (size_t i = 0; i < rot.size(); i++) {
            t.rot4[i] = mfm_pack16(mfm_lo16(rot[i].x), mfm_lo16(rot[i].y)); /* {(rr, -ri), (ri, rr)} -> (rr, ri) */
        }
        rot.clear();
    }
    return MFM_OK;
}

} /* namespace */

int build_host_tables(const KernelPlan &p, std::vector<Channel> &chans, HostTables &t)
{
    build_dot2_taps(p, chans, t);
    if (p.variant >= 1u) {
        build_fragments(p, chans, t);
    }
    const int rc = build_rotators(p, chans, t);
    if (rc != MFM_OK) {
        return rc;
    }
    t.info.resize((size_t)p.ngroups * MFM_CG);
    memset(t.info.data(), 0, t.info.size() * sizeof(mfm_chan_info));
    for (uint32_t c = 0; c < p.C; c++) {
        const Channel &ch = chans[p.perm[c]];
        mfm_chan_info &in = t.info[c];
        in.rot_base = ch.rot_base;
        in.mu = ch.mu;
        in.lam = ch.lam;
        in.lam_magic = (uint32_t)std::min<uint64_t>(0xffffffffull, (1ull << 32) / ch.lam);
        in.out_row = p.perm[c];
        in.rot_class = chan_class(ch) | (chan_class(ch) != MFM_RC_GENERAL ? chan_turns(ch) << 4 : 0u);
    }
    /* atan LUT: fast_atan2f.c:14-81, entries atan(i/255) at 7 significant digits */
    float tbl[257];
    mfm_hosttwin_atan_table(tbl);
    if (!mfm_hosttwin_atan_table_ok()) {
        return fail(MFM_E_INVAL, "atan table self-check failed (host libm rounds atan() differently)");
    }
    t.lut.resize(256);
    for (int i = 0; i < 256; i++) {
        t.lut[i] = make_float2(tbl[i], tbl[i + 1] - tbl[i]);
    }
    return MFM_OK;
}
