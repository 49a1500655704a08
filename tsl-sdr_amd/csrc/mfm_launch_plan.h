/*
 * mfm_launch_plan.h - what one launch of the channel engine (mfm_engine.hip, launch_locked) does, decided from the engine's
 * scalars alone: how many outputs, which stream, who carries the unconsumed samples and from where, how the tiles are cut
 * into chunks.  Plain C++17, no HIP runtime and no device types: launch_locked() gathers a LaunchInput, calls launch_plan()
 * and queues what the LaunchPlan says; tests/test_launch_plan.py compiles this header with g++ and checks, without a GPU,
 * the arithmetic the two-stream path is safe by.
 */
#pragma once

#include <stdint.h>

#include <algorithm>

/* mfm_kernel.h's MFM_V3_OT and MFM_V3_LEAD (that header names device types; mfm_engine.hip asserts the equality) */
constexpr uint32_t LP_V3_OT = 64u, LP_V3_LEAD = 4u;
constexpr uint32_t LP_CUS = 256u; /* workgroup slots = LP_CUS * workgroups per CU */

/* the outputs n_avail samples give: one per D once the T taps are covered.  THE count - the engine has no other copy of it. */
inline uint32_t launch_outputs(uint64_t n_avail, uint32_t T, uint32_t D)
{
    return n_avail >= T ? (uint32_t)((n_avail - T) / D + 1u) : 0u;
}

/* ---- accepting a block (plan_block): what nr_samples more in the buffer being filled would mean ---- */

struct AcceptPlan {
    uint64_t pend_after = 0; /* accepted and not launched, this block included */
    uint32_t n_new = 0;      /* outputs a launch would then give */
    bool must = false;       /* the buffer has to be launched once this block is in (no coalescing, or coalesce_samples gathered) */
    bool policy = false;     /* it need not, but could: accept_wants() decides from the launches in flight */
};

inline AcceptPlan accept_plan(uint32_t T, uint32_t D, uint32_t tail, uint32_t pend, uint64_t nr_samples, uint32_t coalesce_samples,
                              bool gather)
{
    AcceptPlan a;
    a.pend_after = (uint64_t)pend + nr_samples;
    a.n_new = launch_outputs((uint64_t)tail + a.pend_after, T, D);
    a.must = 0 == coalesce_samples || a.pend_after >= coalesce_samples;
    a.policy = !a.must && a.n_new && !gather;
    return a;
}

/* the policy of mfm_engine_config::coalesce_samples: launch although it does not have to when nothing is in flight, or when one
 * launch is and a quarter of what it read has gathered (in_flight: 0, 1, or 2 for "two or more") */
inline bool accept_wants(const AcceptPlan &a, int in_flight, uint32_t last_launch_samples)
{
    return a.policy && (0 == in_flight || (1 == in_flight && 4u * a.pend_after >= last_launch_samples));
}

/* ---- one launch ---- */

struct LaunchInput {
    uint32_t T = 0, D = 0;   /* taps, decimation */
    uint32_t variant = 0;    /* 0 dot2, 1 first-generation matrix kernel, 2 second-generation */
    bool raw8 = false;       /* the buffer holds 8-bit blocks as they came off the wire */
    uint32_t hist = 0, tail = 0, pend = 0; /* mfm_engine's: the buffer is [hist | tail | pend] */
    uint32_t ncs = 1;        /* compute streams */
    bool auto_alt = false;   /* two streams without having been asked (int16 blocks only) */
    bool ring = false;       /* the carry ring exists */
    bool head = false;       /* this buffer's [hist | tail] is in a ring slot, not at its front */
    /* workgroups per CU of the alternation rule (KernelPlan::v_wg_per_cu) and of the chunking and the grid (FormatPlan::wg_per_cu,
     * the buffer's input format: the long-filter kernel's small 8-bit instances run two per CU where the plan says one) */
    uint32_t alt_wg_per_cu = 1, wg_per_cu = 1;
    uint32_t nslices = 1;    /* channel slices of the kernel description launched (one number for every format: fill_v3, mfm_plan.hip) */
    uint32_t opl = 2;        /* dot2: outputs per lane */
    uint32_t ot = 0;         /* first generation: outputs per tile */
};

enum LaunchHead {
    LP_HEAD_NONE = 0,  /* the buffer's front is where it always was */
    LP_HEAD_KERNEL,    /* the kernel reads its first head_n samples from the ring slot (mfm_launch_v3::head) */
    LP_HEAD_COPY_BACK, /* the ring slot is copied to the buffer's front first */
};

enum LaunchCarrier {
    LP_CARRY_NONE = 0, /* nothing to carry */
    LP_CARRY_KERNEL,   /* the channel kernel, behind its last tile (tail_src, tail_n) */
    LP_CARRY_COPY,     /* a copy on the stream of the NEXT launch */
    LP_CARRY_RING,     /* the ring kernel on the input stream, into the next pass's ring slot */
};

struct LaunchPlan {
    uint32_t n_avail = 0, n_new = 0;
    /* The launch after this one goes to the other compute stream.  Two streams pay off when a launch fills the workgroup slots
     * more than once (its ragged end is what the next launch moves into); a launch of one tile per slot or less costs more in the
     * extra packets of the carry (a copy, two events) than it gains: it keeps the carry in the kernel and the next launch stays
     * behind it on the same stream.  An engine that alternates without having been asked to does so for int16 blocks only.
     * And only when what its carry reads - the last consumed row and the unconsumed samples behind it - lies behind the
     * [hist | tail] front of this buffer, which the previous launch's carry wrote on the OTHER stream (n_new * D >= tail + D:
     * carry_src >= hist + tail): the carry is then ordered behind everything it reads (the H2D copies, through in_ready)
     * without a wait of its own.  True for every launch of more than a tile per slot; spelled out so that it does not rest on
     * that. */
    bool two = false;
    /* Early carry: an alternating launch of int16 blocks leaves the next launch's [hist | tail] in the carry ring instead of at
     * the front of the next buffer, copied at submit time by a one-workgroup kernel on the input stream - behind the producer of
     * this block and behind no channel kernel.  `two` says that what is copied lies behind this buffer's first hist + tail
     * samples, in what the producer of this block wrote, and the input stream is behind that producer (submit_impl).
     * NO EVENT GUARDS A RING SLOT.  Pass r of launch_locked() reads buffer r % nbuf and, if its head is in the ring, slot
     * r % (nbuf + 1); it writes slot (r + 1) % (nbuf + 1), which pass r + 1 - (nbuf + 1) = r - nbuf read last; that pass also
     * read buffer (r - nbuf) % nbuf = r % nbuf, the buffer of pass r, and acquire_input() has waited on the host for its
     * kernel's end (in_free) before the producer of pass r's block was allowed to write - so before this submit.  (Two
     * buffers: slot (r + 1) % 3 was last read by launch r - 2.)  A slot holds 2 * D + T + 16 samples; carry_n < D + T. */
    bool early = false;
    /* A head in the ring: the kernel takes it from there when it alternates (a launch that does not carries the tail itself,
     * out of the buffer's front, or there is no kernel at all) and when nothing but the prologue of a first chunk's workgroup
     * reads the first head_n samples: the second tile's image starts (OT - LEAD) rows into the buffer, and no workgroup comes to
     * a first chunk as its second item (nitems <= slots).  Both hold wherever `two` does today; spelled out so that the kernel's
     * assumption does not rest on that.  Otherwise the samples go where they would have been: nobody reads this buffer's front
     * any more, acquire_input() has waited for the launch that did. */
    LaunchHead head = LP_HEAD_NONE;
    uint32_t head_n = 0; /* hist + tail when there is a head */
    /* Second generation: nchunks chunks of cl consecutive tiles (lengths equal to within one tile; a chunk pays one extra column
     * group), one chunk per workgroup slot and slice - shorter chunks, several rounds, were 2-6 % slower on MI355X.  nchunks per
     * slice is a multiple of 8 where there are 8 slots: the items are dealt chunk-major over the eight XCDs - item = 8 * (chunk /
     * 8 * nslices + slice) + chunk % 8, mfm3_decode_item - so a chunk count that is not one leaves holes in the last group of
     * eight, the grid overflows the slots and a few workgroups run a SECOND chunk while the others are done: with 3, 5, 6 or 12
     * slices (130-192, 257-320, ... channels) a launch took up to twice as long as its work, profiles/r06_ab_chunking.txt.
     * The other kernels: every tile its own chunk; dot2 launches an item per workgroup whatever the slots. */
    uint32_t ntiles = 0, nchunks = 0, cl = 0, nitems = 0, grid = 0;
    /* who takes the next launch's [hist | history tail] - the last consumed row (second generation) and what was not consumed -
     * to where the next launch reads it, and its range in this buffer, in samples */
    LaunchCarrier carrier = LP_CARRY_NONE;
    uint32_t carry_src = 0, carry_n = 0;
    /* the kernel description's own fields: the first generation carries what was not consumed and nothing in front of it; the
     * second, when it alternates, nothing (the next launch must not wait for this kernel) */
    uint32_t tail_src = 0, tail_n = 0;
    uint32_t new_hist = 0, new_tail = 0; /* mfm_engine::hist, ::tail behind this launch */
    /* this launch, or its stream's copy, writes the carry into the next buffer: whoever read that one last - possibly on the
     * other stream - must be through */
    bool wait_next_reader = false;
};

inline LaunchPlan launch_plan(const LaunchInput &in)
{
    LaunchPlan p;
    const uint32_t D = in.D;
    const bool v3 = 2u == in.variant;
    p.n_avail = in.tail + in.pend;
    p.n_new = launch_outputs(p.n_avail, in.T, D);
    if (in.ncs > 1u && v3 && p.n_new && !(in.auto_alt && in.raw8)) {
        const uint32_t ntiles = (p.n_new + LP_V3_OT - 1u) / LP_V3_OT, slots = LP_CUS * in.alt_wg_per_cu;
        p.two = (uint64_t)ntiles * in.nslices > slots && (uint64_t)p.n_new * D >= (uint64_t)in.tail + D;
    }
    p.early = p.two && !in.raw8 && in.ring;
    p.wait_next_reader = in.ncs > 1u && !p.two;

    const uint32_t slots = LP_CUS * in.wg_per_cu;
    if (p.n_new && v3) {
        p.ntiles = (p.n_new + LP_V3_OT - 1u) / LP_V3_OT;
        uint32_t per_slice = std::max(1u, slots / in.nslices);
        per_slice = per_slice >= 8u ? per_slice & ~7u : per_slice;
        p.nchunks = std::min(p.ntiles, per_slice);
        p.cl = (p.ntiles + p.nchunks - 1u) / p.nchunks;
        p.nitems = ((p.nchunks + 7u) / 8u) * 8u * in.nslices;
        p.grid = std::min(p.nitems, slots);
    } else if (p.n_new) {
        const uint32_t ot = 1u == in.variant ? in.ot : 64u * in.opl - 1u; /* (dot2: a tile's last output is the next one's first) */
        p.ntiles = (p.n_new + ot - 1u) / ot;
        p.nchunks = p.ntiles;
        p.cl = 1u;
        p.nitems = ((p.ntiles + 7u) / 8u) * 8u * in.nslices;
        p.grid = 1u == in.variant ? std::min(p.nitems, slots) : p.nitems;
    }

    if (in.head) {
        p.head_n = in.hist + in.tail;
        p.head = (p.two && !in.raw8 && p.head_n <= (LP_V3_OT - LP_V3_LEAD) * D && p.nitems <= slots) ? LP_HEAD_KERNEL : LP_HEAD_COPY_BACK;
    }

    const uint32_t consumed = p.n_new * D;
    p.new_tail = p.n_avail - consumed;
    /* the second generation recomputes the output in front of a launch from the last consumed row instead of reading carried
     * state (mfm_launch_v3::hist): D once the stream has produced an output, and what it was before */
    p.new_hist = (v3 && p.n_new) ? D : in.hist;
    p.carry_src = in.hist + consumed - p.new_hist;
    p.carry_n = p.new_hist + p.new_tail;
    if (p.n_new && v3) {
        p.tail_src = p.carry_src;
        p.tail_n = p.two ? 0u : p.carry_n;
    } else if (p.n_new && 1u == in.variant) {
        p.tail_src = consumed;
        p.tail_n = p.new_tail;
    }
    if (p.early) {
        p.carrier = LP_CARRY_RING;
    } else if (p.n_new && (v3 ? !p.two : 1u == in.variant)) {
        p.carrier = LP_CARRY_KERNEL;
    } else if (p.carry_n) {
        p.carrier = LP_CARRY_COPY;
    }
    return p;
}
