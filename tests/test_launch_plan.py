"""What one launch of the channel engine does (tsl-sdr_amd/csrc/mfm_launch_plan.h: launch_plan, the decisions launch_locked()
queues) on the host: the header is plain C++17, so g++ builds a checker around it and no GPU is involved.

  * Boundaries: at every threshold of the rule - the first output, one tile per workgroup slot and slice, a carry that starts
    at the [hist | tail] front, 8-bit blocks on an engine that alternates unasked, the ring, a head as long as the first tile's
    lead, more first chunks than slots, the rounding of the chunks per slice to eight - the planner is compared, on both sides,
    with a restatement written here from the rule as tests/test_overlap_forms.py's docstring and DESIGN.md 3.2 state it.
  * Invariants, over the whole product of the shapes and the sample counts around every one of those boundaries: the
    arithmetic the two-stream path is safe by, which the engine only ever stated in comments - above all that an early carry
    reads behind this buffer's first hist + tail samples (no event orders it behind the copy that wrote them) and fits a ring
    slot of 2 * D + T + 16 samples (launch_locked()'s MFM_E_STATE cannot be reached from a plan).

That the engine queues what the plan says is what the GPU tests pin (tests/test_overlap_forms.py, test_launch_overlap.py,
test_coalesce.py)."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OT, LEAD, CUS = 64, 4, 256            # outputs per tile and lead rows of the second generation, compute units
DS = (1, 4, 25, 96)
SLICES = (1, 3, 16)
FIELDS = ("n_avail n_new two early head head_n ntiles nchunks cl nitems grid carrier carry_src carry_n tail_src tail_n "
          "new_hist new_tail wait_next_reader").split()
HEAD_NONE, HEAD_KERNEL, HEAD_COPY_BACK = 0, 1, 2
CARRY_NONE, CARRY_KERNEL, CARRY_COPY, CARRY_RING = 0, 1, 2, 3


def _taps(D):
    """taps below the decimation are refused at commit"""
    return sorted({t for t in (D, D + 1, 128, 150) if t >= D})


CHECKER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include "mfm_launch_plan.h"

static long bad = 0, checked = 0;
static void show(const LaunchInput &i)
{
    printf(" [T %u D %u variant %u raw8 %d hist %u tail %u pend %u ncs %u auto_alt %d ring %d head %d alt_wg %u wg %u nslices %u]\n", i.T, i.D,
           i.variant, i.raw8, i.hist, i.tail, i.pend, i.ncs, i.auto_alt, i.ring, i.head, i.alt_wg_per_cu, i.wg_per_cu, i.nslices);
}
#define REQUIRE(c, what) do { if (!(c)) { if (bad++ < 40) { printf("FAIL %s:", what); show(in); } } } while (0)

static void invariants(const LaunchInput &in)
{
    const LaunchPlan p = launch_plan(in);
    const uint64_t D = in.D, T = in.T, slots = 256u * in.wg_per_cu;
    const bool v12 = in.variant == 1 || in.variant == 2;
    checked++;
    REQUIRE(p.n_avail == in.tail + in.pend, "n_avail");
    REQUIRE((uint64_t)p.n_new * D + p.new_tail == p.n_avail && p.new_tail < T, "n_new * D + new_tail == n_avail, new_tail < T");
    REQUIRE(p.n_new == launch_outputs(p.n_avail, in.T, in.D), "one output count");
    if (p.n_new == 0) {
        REQUIRE(!p.two && p.ntiles == 0 && p.nitems == 0 && p.grid == 0 && p.carrier != LP_CARRY_KERNEL && p.head != LP_HEAD_KERNEL && p.tail_n == 0,
                "no outputs: no kernel, one stream");
        REQUIRE(p.new_hist == in.hist, "no outputs: hist stays");
    }
    REQUIRE(!p.two || (in.variant == 2 && p.n_new > 0 && in.ncs > 1), "two implies the second generation, outputs, two streams");
    REQUIRE(!p.early || (p.two && !in.raw8 && in.ring), "early implies two, int16, a ring");
    REQUIRE(p.new_hist == (in.variant == 2 && p.n_new ? in.D : in.hist), "new_hist");
    REQUIRE(p.carry_n == p.new_hist + p.new_tail, "carry_n");
    if (p.carry_n > 0) {
        REQUIRE(p.carrier != LP_CARRY_NONE, "somebody carries");
    }
    REQUIRE((p.carrier == LP_CARRY_KERNEL) == (p.n_new > 0 && !p.two && v12), "the kernel carries iff it runs, does not alternate, variant 1 or 2");
    REQUIRE((p.carrier == LP_CARRY_RING) == p.early, "the ring carries iff early");
    REQUIRE(p.carrier != LP_CARRY_NONE || p.carry_n == 0, "nobody carries nothing");
    REQUIRE((uint64_t)p.carry_src + p.carry_n <= (uint64_t)in.hist + p.n_avail, "the carry reads inside the buffer");
    if (p.carrier == LP_CARRY_KERNEL) {
        REQUIRE(p.tail_n == (in.variant == 2 ? p.carry_n : p.new_tail) && (uint64_t)p.tail_src + p.tail_n == (uint64_t)in.hist + p.n_avail,
                "the kernel's own carry ends at the buffer's end");
    } else {
        REQUIRE(p.tail_n == 0, "a kernel that does not carry has tail_n 0");
    }
    if (p.two) {
        /* the claim the missing event rests on (copy or ring: neither waits for the carry that wrote this buffer's front) */
        REQUIRE((uint64_t)p.carry_src >= (uint64_t)in.hist + in.tail, "an alternating launch's carry starts behind hist + tail");
    }
    if (p.early) {
        REQUIRE((uint64_t)p.carry_n <= 2 * D + T + 16, "an early carry fits a ring slot");
    }
    REQUIRE(p.wait_next_reader == (in.ncs > 1 && !p.two), "wait_next_reader");
    if (p.n_new) {
        REQUIRE(1 <= p.nchunks && p.nchunks <= p.ntiles, "1 <= nchunks <= ntiles");
        REQUIRE(p.cl == (p.ntiles + p.nchunks - 1) / p.nchunks && (uint64_t)p.cl * p.nchunks >= p.ntiles, "cl == ceil(ntiles / nchunks)");
        REQUIRE(p.nitems % (8 * in.nslices) == 0 && p.nitems >= p.nchunks * in.nslices, "nitems: a multiple of 8 * nslices that holds every chunk");
        /* (dot2 is not a persistent kernel: a workgroup per item, whatever the slots) */
        REQUIRE(p.grid == (v12 ? (uint32_t)std::min<uint64_t>(p.nitems, slots) : p.nitems), "grid == min(nitems, slots)");
        const uint32_t ot = in.variant == 2 ? 64u : in.variant == 1 ? in.ot : 64u * in.opl - 1u;
        REQUIRE((uint64_t)p.ntiles * ot >= p.n_new && (uint64_t)(p.ntiles - 1) * ot < p.n_new, "ntiles covers n_new");
    }
    REQUIRE((p.head == LP_HEAD_NONE) == !in.head && p.head_n == (in.head ? in.hist + in.tail : 0), "a head is read or copied back");
    if (p.head == LP_HEAD_KERNEL) {
        REQUIRE(p.two && !in.raw8 && p.head_n <= 60 * D && p.nitems <= slots, "the kernel reads the head only where its prologue alone does");
    }
    if (in.head && !(p.two && !in.raw8 && p.head_n <= 60 * D && p.nitems <= slots)) {
        REQUIRE(p.head == LP_HEAD_COPY_BACK, "otherwise the head is copied back");
    }
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "plans")) {
        /* one LaunchInput per line of stdin, its LaunchPlan per line of stdout */
        LaunchInput in;
        int raw8, auto_alt, ring, head;
        while (scanf("%u %u %u %d %u %u %u %u %d %d %d %u %u %u %u %u", &in.T, &in.D, &in.variant, &raw8, &in.hist, &in.tail, &in.pend, &in.ncs,
                     &auto_alt, &ring, &head, &in.alt_wg_per_cu, &in.wg_per_cu, &in.nslices, &in.opl, &in.ot) == 16) {
            in.raw8 = raw8, in.auto_alt = auto_alt, in.ring = ring, in.head = head;
            const LaunchPlan p = launch_plan(in);
            printf("%u %u %d %d %d %u %u %u %u %u %u %d %u %u %u %u %u %u %d\n", p.n_avail, p.n_new, p.two, p.early, (int)p.head, p.head_n, p.ntiles,
                   p.nchunks, p.cl, p.nitems, p.grid, (int)p.carrier, p.carry_src, p.carry_n, p.tail_src, p.tail_n, p.new_hist, p.new_tail,
                   p.wait_next_reader);
        }
        return 0;
    }
    /* the invariants over the whole product; per shape, n_avail and tail around every boundary */
    /* (slices: the three of the shapes, and those that leave a slice 13, 8 and 6 of 256 slots, 6 of 512) */
    const uint32_t Ds[] = { 1, 4, 25, 96 }, slices[] = { 1, 3, 16, 19, 32, 42, 80 };
    for (uint32_t D : Ds)
    for (uint32_t T : { D, D + 1, 128u, 150u }) if (T >= D)
    for (uint32_t ns : slices)
    for (uint32_t wg = 1; wg <= 2; wg++)
    for (uint32_t variant = 0; variant <= 2; variant++)
    /* the alternation rule's workgroups per CU and mfm_engine::hist are the second generation's: the other kernels have neither */
    for (uint32_t awg = variant == 2 ? 1 : wg; awg <= (variant == 2 ? 2 : wg); awg++)
    for (uint32_t hist : { 0u, D }) if (variant == 2 || hist == 0) {
        const uint32_t ot = variant == 2 ? 64u : variant == 1 ? 32u : 127u;
        std::set<uint32_t> outs = { 0, 1, 2, ot, ot + 1 };
        for (uint32_t w : { wg, awg }) {
            const uint32_t slots = 256u * w, lo = slots / ns, per = std::max(1u, lo) >= 8 ? lo & ~7u : std::max(1u, lo);
            for (uint32_t nt : { lo, per, slots }) if (nt) {
                outs.insert(nt * ot);
                outs.insert(nt * ot + 1);
            }
        }
        for (uint32_t n_new : outs)
        for (uint32_t extra : { 0u, D - 1 }) {
            const uint32_t n_avail = n_new ? T + (n_new - 1) * D + extra : T - 1 - std::min(extra, T - 1);
            const uint32_t tails[] = { 0, 1, T - 1, n_new * D - D, n_new * D - D + 1, 60 * D - hist, 60 * D - hist + 1, n_avail };
            for (uint32_t tail : tails) if (tail <= n_avail && (n_new || tail != n_new * D - D + 1))
            for (int flags = 0; flags < 32; flags++) {
                LaunchInput in;
                in.T = T, in.D = D, in.variant = variant, in.hist = hist, in.tail = tail, in.pend = n_avail - tail;
                in.raw8 = flags & 1, in.auto_alt = flags & 2, in.ring = flags & 4, in.head = flags & 8, in.ncs = flags & 16 ? 2 : 1;
                in.alt_wg_per_cu = awg, in.wg_per_cu = wg, in.nslices = ns, in.opl = 2, in.ot = 32;
                invariants(in);
            }
        }
    }
    {
        /* accepting a block (plan_block): the same output count; the coalescing policy on both sides of its thresholds */
        LaunchInput in;
        in.T = 128, in.D = 96;
        AcceptPlan a = accept_plan(128, 96, 100, 20, 7, 0, false);
        REQUIRE(a.pend_after == 27 && a.n_new == 0 && a.must && !a.policy, "127 samples, no coalescing");
        a = accept_plan(128, 96, 100, 20, 8, 0, false);
        REQUIRE(a.n_new == 1 && a.must && !a.policy && !accept_wants(a, 0, 0), "128 samples, no coalescing: must, and no policy");
        a = accept_plan(128, 96, 100, 20, 980, 1000, false);
        REQUIRE(a.pend_after == 1000 && a.must && !a.policy, "coalesce_samples gathered");
        a = accept_plan(128, 96, 100, 20, 979, 1000, false);
        REQUIRE(a.pend_after == 999 && a.n_new == 11 && !a.must && a.policy, "one sample short of coalesce_samples");
        REQUIRE(accept_wants(a, 0, 1u << 30) && accept_wants(a, 1, 3996) && !accept_wants(a, 1, 3997) && !accept_wants(a, 2, 0),
                "nothing in flight, or one launch and a quarter of what it read");
        a = accept_plan(128, 96, 100, 20, 979, 1000, true);
        REQUIRE(!a.must && !a.policy && !accept_wants(a, 0, 0), "MFM_F_GATHER: no policy");
        a = accept_plan(128, 96, 100, 20, 7, 1000, false);
        REQUIRE(!a.must && !a.policy && !accept_wants(a, 0, 0), "no outputs: no policy");
        checked += 7;
    }
    printf("checked %ld inputs, %ld failures\n", checked, bad);
    return bad ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("launch_plan")
    src, exe = d / "check_launch_plan.cpp", d / "check_launch_plan"
    src.write_text(CHECKER)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tsl-sdr_amd", "csrc"), "-o", str(exe), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def test_the_header_compiles_alone(tmp_path):
    """no HIP runtime, no device types: g++ takes the header by itself"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "mfm_launch_plan.h"\nint main() { return (int)launch_plan(LaunchInput()).n_new; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tsl-sdr_amd", "csrc"), "-o",
                        str(tmp_path / "alone"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]


def test_invariants_over_the_product_of_shapes(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "checked" and int(last[1]) > 1000000 and int(last[3]) == 0, r.stdout[-400:]


# ------------------------------------------------------------------------------------------------ the rule, restated

def _restate(i):
    """The plan of one launch from the rule in words (tests/test_overlap_forms.py), not from the header:

        n_new   = (n_avail - T) // D + 1 once the taps are covered
        a launch alternates iff the engine has two streams, runs the second-generation kernel, has outputs, is not an 8-bit
        launch of an engine that alternates unasked, and ntiles * nslices > slots and n_new * D >= tail + D
        its carry goes to the ring iff it alternates, reads int16 and there is a ring
        chunks: one per workgroup slot and slice, in eights per slice where a slice has eight slots; items in eights per slice
        a head in the ring is read by the kernel iff the launch alternates, reads int16, the head ends inside the first tile's
        image ((OT - LEAD) * D samples) and no workgroup runs two items; otherwise it goes back to the buffer's front
        carried: the unconsumed samples and, on the second generation once it has produced an output, the D samples in front."""
    T, D, v = i["T"], i["D"], i["variant"]
    avail = i["tail"] + i["pend"]
    n_new = (avail - T) // D + 1 if avail >= T else 0
    ot = {0: 64 * i["opl"] - 1, 1: i["ot"], 2: OT}[v]
    ntiles = -(-n_new // ot)
    two = (i["ncs"] > 1 and v == 2 and n_new > 0 and not (i["auto_alt"] and i["raw8"])
           and ntiles * i["nslices"] > CUS * i["alt_wg"] and n_new * D >= i["tail"] + D)
    early = two and not i["raw8"] and i["ring"]
    slots = CUS * i["wg"]
    if n_new == 0:
        nchunks = cl = nitems = grid = 0
    elif v == 2:
        per_slice = max(1, slots // i["nslices"])
        if per_slice >= 8:
            per_slice -= per_slice % 8
        nchunks = min(ntiles, per_slice)
        cl = -(-ntiles // nchunks)
        nitems = -(-nchunks // 8) * 8 * i["nslices"]
        grid = min(nitems, slots)
    else:
        nchunks, cl = ntiles, 1
        nitems = -(-ntiles // 8) * 8 * i["nslices"]
        grid = min(nitems, slots) if v == 1 else nitems
    head, head_n = HEAD_NONE, 0
    if i["head"]:
        head_n = i["hist"] + i["tail"]
        head = HEAD_KERNEL if two and not i["raw8"] and head_n <= (OT - LEAD) * D and nitems <= slots else HEAD_COPY_BACK
    new_tail = avail - n_new * D
    new_hist = D if v == 2 and n_new else i["hist"]
    carry_n = new_hist + new_tail
    carry_src = i["hist"] + avail - carry_n
    if early:
        carrier = CARRY_RING
    elif n_new and v in (1, 2) and not two:
        carrier = CARRY_KERNEL
    else:
        carrier = CARRY_COPY if carry_n else CARRY_NONE
    tail_src = tail_n = 0
    if n_new and v == 2:
        tail_src, tail_n = carry_src, (0 if two else carry_n)     # the last consumed row and what was not consumed
    elif n_new and v == 1:
        tail_src, tail_n = n_new * D, new_tail                    # what was not consumed
    return dict(n_avail=avail, n_new=n_new, two=int(two), early=int(early), head=head, head_n=head_n, ntiles=ntiles, nchunks=nchunks,
                cl=cl, nitems=nitems, grid=grid, carrier=carrier, carry_src=carry_src, carry_n=carry_n, tail_src=tail_src, tail_n=tail_n,
                new_hist=new_hist, new_tail=new_tail, wait_next_reader=int(i["ncs"] > 1 and not two))


def _avail_for(n_new, T, D, extra=0):
    """n_avail that gives n_new outputs (extra < D more samples give no more); n_new 0: one sample short of the first"""
    return T + (n_new - 1) * D + extra if n_new else T - 1


def _boundary_cases():
    """every boundary, both sides, on every shape; each case is (what it is, what must come out, the input)"""
    cases = []

    def add(what, expect, **kw):
        i = dict(T=0, D=0, variant=2, raw8=0, hist=0, tail=0, pend=0, ncs=2, auto_alt=0, ring=1, head=0, alt_wg=1, wg=1, nslices=1,
                 opl=2, ot=32)
        i.update(kw)
        i["pend"] = i.pop("n_avail") - i["tail"]
        assert i["pend"] >= 0, (what, i)
        cases.append((what, expect, i))

    for D, nslices, wg in itertools.product(DS, SLICES, (1, 2)):
        for T in _taps(D):
            slots = CUS * wg
            sh = dict(T=T, D=D, nslices=nslices, wg=wg, alt_wg=wg)
            lo = slots // nslices                 # tiles: lo * nslices <= slots < (lo + 1) * nslices
            big = (lo + 3) * OT                   # outputs of a launch that alternates
            for variant in (0, 1, 2):
                for hist in ((0, D) if variant == 2 else (0,)):       # (mfm_engine::hist is the second generation's)
                    # no output, one output, still one output
                    for n_avail, n_new in ((T - 1, 0), (T, 1), (T + D - 1, 1)):
                        add("first output", dict(n_new=n_new, two=0, new_hist=(D if variant == 2 and n_new else hist)),
                            variant=variant, hist=hist, n_avail=n_avail, **sh)
                # variants 0 and 1 never alternate, however large the launch
                add("variant", dict(two=int(variant == 2)), variant=variant, n_avail=_avail_for(big, T, D), **sh)
            # one tile per slot and slice, and one more (with one slice: ntiles * nslices == slots and slots + 1)
            for extra in (0, D - 1):
                add("tiles == slots", dict(two=0, ntiles=lo), n_avail=_avail_for(lo * OT, T, D, extra), **sh)
                add("tiles > slots", dict(two=1, ntiles=lo + 1), n_avail=_avail_for(lo * OT + 1, T, D, extra), **sh)
            # the two workgroup counts are the alternation rule's and the chunking's, each its own
            for alt_wg, this_wg in itertools.product((1, 2), (1, 2)):
                add("alt_wg", dict(two=int(alt_wg == 1), ntiles=CUS + 1, nchunks=min(CUS + 1, CUS * this_wg)),
                    n_avail=_avail_for(CUS * OT + 1, T, D), **dict(sh, alt_wg=alt_wg, wg=this_wg, nslices=1))
            # the carry starts at the [hist | tail] front, or one sample in front of it
            n_avail = _avail_for(big, T, D)
            add("n_new * D == tail + D", dict(two=1, carry_src=D + big * D - D), hist=D, tail=big * D - D, n_avail=n_avail, **sh)
            add("n_new * D == tail + D - 1", dict(two=0), hist=D, tail=big * D - D + 1, n_avail=n_avail, **sh)
            # 8-bit blocks: on one stream where the engine alternates unasked, on two where it was asked; never early
            add("raw8, unasked", dict(two=0, early=0, carrier=CARRY_KERNEL), raw8=1, auto_alt=1, n_avail=n_avail, **sh)
            add("raw8, asked", dict(two=1, early=0, carrier=CARRY_COPY), raw8=1, auto_alt=0, n_avail=n_avail, **sh)
            add("int16, unasked", dict(two=1, early=1, carrier=CARRY_RING), raw8=0, auto_alt=1, n_avail=n_avail, **sh)
            # the ring
            add("ring", dict(two=1, early=1, carrier=CARRY_RING), ring=1, n_avail=n_avail, **sh)
            add("no ring", dict(two=1, early=0, carrier=CARRY_COPY), ring=0, n_avail=n_avail, **sh)
            add("one stream", dict(two=0, early=0, carrier=CARRY_KERNEL, wait_next_reader=0), ncs=1, n_avail=n_avail, **sh)
            # a head as long as the lead of the second tile's image, and one sample longer
            for hist in (0, D):
                edge = (OT - LEAD) * D
                add("head_n == (OT - LEAD) * D", dict(head=HEAD_KERNEL, head_n=edge), head=1, hist=hist, tail=edge - hist,
                    n_avail=n_avail + edge, **sh)
                add("head_n one more", dict(head=HEAD_COPY_BACK, head_n=edge + 1), head=1, hist=hist, tail=edge - hist + 1,
                    n_avail=n_avail + edge, **sh)
                add("head, one stream", dict(head=HEAD_COPY_BACK), head=1, ncs=1, hist=hist, tail=T - 1, n_avail=n_avail, **sh)
                add("head, no outputs", dict(head=HEAD_COPY_BACK, n_new=0), head=1, hist=hist, tail=T - 1, n_avail=T - 1, **sh)
            add("no head", dict(head=HEAD_NONE, head_n=0), head=0, hist=D, tail=T - 1, n_avail=n_avail, **sh)

    # chunks per slice: below 8 as they are, 8, and 13 rounded down to 8; items equal to the slots and above them
    for D, wg in itertools.product(DS, (1, 2)):
        T, slots = _taps(D)[-1], CUS * wg
        short = min(T - 1, (OT - LEAD) * D - D)     # a head that the kernel may read: hist + tail <= (OT - LEAD) * D
        for per, chunks in ((6, 6), (8, 8), (13, 8), (16, 16)):
            nslices = slots // per
            assert slots // nslices == per
            sh = dict(T=T, D=D, nslices=nslices, wg=wg, alt_wg=wg, head=1, hist=D, tail=short)
            nitems = -(-chunks // 8) * 8 * nslices
            for ntiles in (chunks, chunks + 1, 3 * chunks + 1):
                two = int(ntiles * nslices > slots)
                add(f"per_slice {per}", dict(nchunks=chunks, cl=-(-ntiles // chunks), nitems=nitems, grid=min(nitems, slots), two=two,
                                             head=(HEAD_KERNEL if two and nitems <= slots else HEAD_COPY_BACK)),
                    n_avail=_avail_for(ntiles * OT, T, D), **sh)
            add(f"per_slice {per}, few tiles", dict(nchunks=chunks - 1, nitems=nitems), n_avail=_avail_for((chunks - 1) * OT, T, D), **sh)
        # one slice, eight chunks' worth of slots: nitems == slots
        add("nitems == slots", dict(nitems=slots, grid=slots, head=HEAD_KERNEL), n_avail=_avail_for((slots + 1) * OT, T, D), T=T, D=D,
            wg=wg, alt_wg=wg, head=1, hist=D, tail=short)
    return cases


def test_boundaries_against_the_restated_rule(checker):
    cases = _boundary_cases()
    keys = "T D variant raw8 hist tail pend ncs auto_alt ring head alt_wg wg nslices opl ot".split()
    text = "".join(" ".join(str(i[k]) for k in keys) + "\n" for _, _, i in cases)
    r = subprocess.run([checker, "plans"], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(cases) > 3000
    for (what, expect, i), line in zip(cases, lines):
        got = dict(zip(FIELDS, (int(x) for x in line.split())))
        want = _restate(i)
        assert got == want, (what, i, {k: (got[k], want[k]) for k in FIELDS if got[k] != want[k]})
        # ... and the case lies on the side of the boundary it was built for
        assert all(got[k] == val for k, val in expect.items()), (what, i, expect, got)
