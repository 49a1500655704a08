/*
 * mfm_plan.h - which channel kernel an engine runs and with what geometry, decided on the host from the configuration and
 * the taps alone (mfm_plan.hip), and the host tables that kernel reads.  No device pointers, no HIP runtime calls: the
 * engine's commit (mfm_engine.hip) uploads the tables, fills the device pointers into the plan's launch descriptions and
 * launches through them; mfm_hosttwin_kernel_form() runs the same planner without a device.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <vector>

#include "../../include/multifm_hip.h"
#include "mfm_kernel.h"

struct Channel {
    std::vector<int16_t> cre, cim;
    int16_t incr_re = 0, incr_im = 0;
    bool want_iq = false;
    /* rotator table placement (build_host_tables) */
    uint64_t rot_base = 0;
    uint32_t mu = 0, lam = 1;
};

inline uint64_t input_capacity(uint32_t max_block, uint32_t coalesce, uint32_t nr_taps)
{
    /* history tail (< nr_taps samples) + block + one 16-byte staging chunk of slack (a chunk that starts on the last
     * real sample must still be readable in place: decimations that are not multiples of 4 start their chunks at any
     * sample), rounded to 64 samples.  A coalescing engine launches once coalesce_samples have gathered: fewer than that
     * plus one more block of any size always fit. */
    return ((uint64_t)max_block + coalesce + 2ull * nr_taps + 4u + 63u) & ~63ull; /* 2 x: history tail + mfm_engine::hist (<= taps) */
}

/* what runs blocks of one input format (MFM_IN_*) */
struct FormatPlan {
    const void *kfn = nullptr; /* the kernel instance; nullptr: blocks of this format are widened to int16 first */
    uint32_t lds_bytes = 0, wg_per_cu = 1;
    bool taps_resident = false;
    /* the geometry half of the launch description of the chosen variant: everything but the device pointers (commit) and
     * the block (input address and counts, chunking, output slot, carried state: launch) */
    mfm_launch L{};        /* v_dot2 kernel (int16 blocks only) */
    mfm_launch_mfma M{};   /* first-generation matrix kernel */
    mfm_launch_v3 V{};     /* second generation */
};

struct KernelPlan {
    uint32_t variant = 0; /* mfm_stats::kernel_variant: 0 v_dot2, 1 first-generation matrix kernel, 2 second generation */
    uint32_t T = 0, D = 0, C = 0;
    bool any_iq = false;
    uint32_t cap_in = 0;     /* samples per input buffer */
    uint32_t out_stride = 0; /* outputs per channel one submit can produce (even) */
    uint32_t ngroups = 0;    /* channel groups of MFM_CG (tap table, carried state) */

    /* v_dot2 kernel */
    int opl = 2;
    uint32_t rs2 = 0, lds_bytes = 0, lut_off = 0, nchunks = 0, gpw = 0, nslices = 0;

    /* matrix kernels (mfm_kernel_mfma.hip): the tap fragments and row constants of both generations */
    uint32_t m_ks = 0, m_kq_used = 0; /* k-steps laid out / holding taps at all */
    uint32_t m_row_bytes = 0, m_nstage = 0, m_ot = 0, m_rs = 0, m_plane_bytes = 0, m_lut_off = 0, m_nrb = 0, m_nslices = 0,
             m_lds_bytes = 0, m_wg_per_cu = 1;
    bool m_fixed_planes = false;
    uint32_t m_ah_mask = 0; /* k-steps whose high-byte tap plane is not all zero */

    /* second generation (mfm_kernel_v3.hip; layout 3: mfm_kernel_v3l.hip) */
    uint32_t v_layout = 0, v_rs = 0, v_sp_pitch = 0, v_nstage4 = 0, v_lds_bytes = 0, v_wg_per_cu = 1;
    uint32_t v_cross[4] = { 0, 0, 0, 0 }, v_within[4] = { 0, 0, 0, 0 };
    uint32_t v_t_per = 0, v_t_pitch = 0; /* layout 1: chunk rows */
    uint32_t v_plane = 0, v_ng = 0, v_nstage_p = 0, v_sta_bytes = 0, v_rb = 1; /* layout 3 */
    uint32_t v_shift = 0, v_copy_pitch = 0; /* decimations 1, 2, 4: 8 / D shifted copies of the image, this many bytes apart */
    uint32_t v_nslices = 0; /* channel slices of the second-generation launches: of 64 channels, or of 128 (v_rb = 2) */
    uint32_t v_kq = 0, v_nh = 0, v_kperm[4] = { 0, 0, 0, 0 }; /* the instance's k-step count, k-steps with a high-byte tap
                                                                 plane, and the order the k-steps are laid out in */

    /* rows: the order the channels' taps are laid out in (by rotator class on the second generation) */
    std::vector<uint32_t> perm;
    uint32_t v_rc = 0; /* the lowest rotator class (MFM_RC_*) among the channels: selects the kernel instance */
    uint32_t rot_exact_channels = 0, rot_fast_slices = 0;
    bool raw8_ok = false; /* the matrix kernels can read 8-bit input as it is (IN8 forms) */

    FormatPlan fmt[4]; /* [MFM_IN_*] */
};

/* the kernel plan of a channel set; MFM_OK or MFM_E_* with mfm_last_error() set.  No HIP runtime calls. */
int plan_channel_kernel(const mfm_engine_config &cfg, const std::vector<Channel> &chans, uint32_t nr_taps, KernelPlan &plan);
/* the form fields of mfm_stats (kernel_variant, slice_channels, taps_resident, outputs_per_tile, k_steps, tap_hi_mask,
 * lds_bytes, rot_exact_channels, rot_fast_slices) */
void plan_form_stats(const KernelPlan &plan, mfm_stats *st);

struct HostTables {
    std::vector<uint32_t> coef, tapoff; /* v_dot2 kernel */
    std::vector<uint32_t> afrag;        /* matrix kernels: A fragments ... */
    std::vector<int32_t> krow;          /* ... row constants of int16 input */
    std::vector<int32_t> krow8[4];      /* ... and of 8-bit input, [MFM_IN_*] (raw8_ok) */
    std::vector<mfm_chan_info> info;
    std::vector<uint2> rot;             /* rotator tables, 8-byte entries ... */
    std::vector<uint32_t> rot4;         /* ... or the 4-byte ones the second generation's build reads (then rot is empty) */
    std::vector<float2> lut;            /* atan table */
};

/* every table the plan's kernel reads; places each channel's rotator table (Channel::rot_base, mu, lam) */
int build_host_tables(const KernelPlan &plan, std::vector<Channel> &chans, HostTables &t);
