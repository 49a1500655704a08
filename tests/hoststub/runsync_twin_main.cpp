/*
 * runsync_twin_main.cpp - the host code of the burst sync stage (csrc/mfm_runsync.hip: the geometry, the run checks, the host
 * twin) under AddressSanitizer and UBSan, as a program of its own: tests/test_runsync.py builds it together with mfm_runsync.hip
 * with -fsanitize=address,undefined on the host side and runs it on a burst Mueller-Muller call it wrote to a file.  Every buffer
 * the twin reads or writes is a heap block of exactly the size the call needs, so a step past either end is reported.  No device
 * is looked for: the twin needs none.
 *
 *   runsync_twin IN STATE OUT
 *   IN    uint32 nr_channels, nr_runs, nr_decisions, max_events, nr_words, words[8], max_distance, bit_rule, flags;
 *         nr_runs struct mfm_runmm_run; nr_decisions int16
 *   STATE nr_channels struct mfm_runsync_state, read and written back
 *   OUT   uint64 nr_runs, nr_words, nr_events; the run records; the bit words; the events
 */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/multifm_hip.h"

static char g_error[512];

extern "C" void mfm_internal_set_error(const char *msg)
{
    snprintf(g_error, sizeof(g_error), "%s", msg);
}

static bool read_file(const char *path, std::vector<unsigned char> &out)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        return false;
    }
    unsigned char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) {
        out.insert(out.end(), buf, buf + n);
    }
    fclose(f);
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 4) {
        fprintf(stderr, "usage: %s IN STATE OUT\n", argv[0]);
        return 2;
    }
    const size_t HEAD = 16 * 4;
    std::vector<unsigned char> in, st;
    if (!read_file(argv[1], in) || !read_file(argv[2], st) || in.size() < HEAD) {
        fprintf(stderr, "cannot read the input\n");
        return 2;
    }
    uint32_t head[16];
    memcpy(head, in.data(), HEAD);
    const size_t nr_runs = head[1], nr_decs = head[2];
    if (in.size() != HEAD + nr_runs * sizeof(mfm_runmm_run) + nr_decs * 2 || st.size() != head[0] * sizeof(mfm_runsync_state)) {
        fprintf(stderr, "the input's sizes do not add up\n");
        return 2;
    }
    std::vector<mfm_runmm_run> runs(nr_runs);
    std::vector<int16_t> decs(nr_decs);
    std::vector<mfm_runsync_state> state(head[0]);
    if (nr_runs) {
        memcpy(runs.data(), in.data() + HEAD, nr_runs * sizeof(mfm_runmm_run));
    }
    if (nr_decs) {
        memcpy(decs.data(), in.data() + HEAD + nr_runs * sizeof(mfm_runmm_run), nr_decs * 2);
    }
    memcpy(state.data(), st.data(), st.size());
    mfm_runsync_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.abi_version = MFM_ABI_VERSION;
    cfg.nr_channels = head[0];
    cfg.max_runs = nr_runs ? (uint32_t)nr_runs : 1u;
    cfg.max_decisions = nr_decs ? (uint32_t)nr_decs : 1u;
    cfg.max_events = head[3];
    cfg.nr_words = head[4];
    memcpy(cfg.words, head + 5, 32);
    cfg.max_distance = head[13];
    cfg.bit_rule = head[14];
    cfg.flags = head[15];
    const uint64_t totals[4] = { nr_runs, nr_decs, 0, 0 };
    if (mfm_hosttwin_runsync_state_check(cfg.nr_channels, state.data()) != MFM_OK) {
        fprintf(stderr, "state: %s\n", g_error);
        return 1;
    }
    /* once without room: the sizes needed, and nothing written */
    size_t nr = 0, nw = 0, ne = 0;
    uint32_t flags = 0;
    const std::vector<mfm_runsync_state> before(state);
    int rc = mfm_hosttwin_runsync_call(&cfg, state.data(), runs.data(), decs.data(), totals, nullptr, 0, &nr, nullptr, 0, &nw, nullptr, 0, &ne,
                                       &flags);
    if (rc != MFM_OK && rc != MFM_E_NOMEM) {
        fprintf(stderr, "refused (%d, flags %u): %s\n", rc, flags, g_error);
        return 1;
    }
    if (rc == MFM_E_NOMEM && memcmp(before.data(), state.data(), st.size()) != 0) {
        fprintf(stderr, "a call without room moved the state\n");
        return 1;
    }
    std::vector<mfm_runsync_run> out_runs(nr);
    std::vector<uint32_t> bits(nw);
    std::vector<mfm_runsync_event> events(ne);
    rc = mfm_hosttwin_runsync_call(&cfg, state.data(), runs.data(), decs.data(), totals, out_runs.data(), nr, &nr, bits.data(), nw, &nw,
                                   events.data(), ne, &ne, &flags);
    if (rc != MFM_OK || nr != out_runs.size() || nw != bits.size() || ne != events.size()) {
        fprintf(stderr, "the second call: %d (%s)\n", rc, g_error);
        return 1;
    }
    if (mfm_hosttwin_runsync_state_check(cfg.nr_channels, state.data()) != MFM_OK) {
        fprintf(stderr, "the state the call left: %s\n", g_error);
        return 1;
    }
    FILE *f = fopen(argv[3], "wb");
    const uint64_t counts[3] = { nr, nw, ne };
    bool ok = f && fwrite(counts, 8, 3, f) == 3 && (!nr || fwrite(out_runs.data(), sizeof(mfm_runsync_run), nr, f) == nr) &&
              (!nw || fwrite(bits.data(), 4, nw, f) == nw) && (!ne || fwrite(events.data(), sizeof(mfm_runsync_event), ne, f) == ne);
    ok = f && fclose(f) == 0 && ok;
    f = fopen(argv[2], "wb");
    ok = f && fwrite(state.data(), 1, st.size(), f) == st.size() && ok;
    ok = f && fclose(f) == 0 && ok;
    printf("{\"runs\": %zu, \"words\": %zu, \"events\": %zu}\n", nr, nw, ne);
    return ok ? 0 : 1;
}
