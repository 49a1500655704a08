/*
 * runbatch_twin_main.cpp - the host code of the burst batch stage (csrc/mfm_runbatch.hip: the geometry, the run and event
 * checks, the host twin) under AddressSanitizer and UBSan, as a program of its own: tests/test_runbatch.py builds it together
 * with mfm_runbatch.hip (and mfm_pocsag.hip, which owns the BCH tables) with -fsanitize=address,undefined on the host side and
 * runs it on a burst sync call it wrote to a file.  Every buffer the twin reads or writes is a heap block of exactly the size
 * the call needs, so a step past either end is reported.  No device is looked for: the twin needs none.
 *
 *   runbatch_twin IN STATE OUT
 *   IN    uint32 nr_channels, nr_runs, nr_bit_words, nr_sync_events, max_events, nr_words, words[8], word_mask, keep_distance;
 *         nr_runs struct mfm_runsync_run; nr_bit_words uint32; nr_sync_events struct mfm_runsync_event
 *   STATE nr_channels struct mfm_runbatch_state, read and written back
 *   OUT   uint64 nr_events; the events
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
    const size_t nr_runs = head[1], nr_bits = head[2], nr_sev = head[3];
    if (in.size() != HEAD + nr_runs * sizeof(mfm_runsync_run) + nr_bits * 4 + nr_sev * sizeof(mfm_runsync_event) ||
        st.size() != head[0] * sizeof(mfm_runbatch_state)) {
        fprintf(stderr, "the input's sizes do not add up\n");
        return 2;
    }
    std::vector<mfm_runsync_run> runs(nr_runs);
    std::vector<uint32_t> bits(nr_bits);
    std::vector<mfm_runsync_event> sev(nr_sev);
    std::vector<mfm_runbatch_state> state(head[0]);
    const unsigned char *at = in.data() + HEAD;
    if (nr_runs) {
        memcpy(runs.data(), at, nr_runs * sizeof(mfm_runsync_run));
    }
    at += nr_runs * sizeof(mfm_runsync_run);
    if (nr_bits) {
        memcpy(bits.data(), at, nr_bits * 4);
    }
    at += nr_bits * 4;
    if (nr_sev) {
        memcpy(sev.data(), at, nr_sev * sizeof(mfm_runsync_event));
    }
    memcpy(state.data(), st.data(), st.size());
    uint64_t decs = 0;
    for (size_t r = 0; r < nr_runs; r++) {
        decs += runs[r].nr_dec;
    }
    mfm_runbatch_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.abi_version = MFM_ABI_VERSION;
    cfg.nr_channels = head[0];
    cfg.max_runs = nr_runs ? (uint32_t)nr_runs : 1u;
    cfg.max_decisions = decs ? (uint32_t)decs : 1u;
    cfg.max_events = head[4];
    cfg.nr_words = head[5];
    memcpy(cfg.words, head + 6, 32);
    cfg.word_mask = head[14];
    cfg.keep_distance = head[15];
    const uint64_t totals[4] = { nr_runs, nr_sev, 0, 0 };
    if (mfm_hosttwin_runbatch_state_check(cfg.nr_channels, state.data()) != MFM_OK) {
        fprintf(stderr, "state: %s\n", g_error);
        return 1;
    }
    /* once without room: the size needed, and nothing written */
    size_t ne = 0;
    uint32_t flags = 0;
    const std::vector<mfm_runbatch_state> before(state);
    int rc = mfm_hosttwin_runbatch_call(&cfg, state.data(), runs.data(), bits.data(), sev.data(), totals, nullptr, 0, &ne, &flags);
    if (rc != MFM_OK && rc != MFM_E_NOMEM) {
        fprintf(stderr, "refused (%d, flags %u): %s\n", rc, flags, g_error);
        return 1;
    }
    if (rc == MFM_E_NOMEM && memcmp(before.data(), state.data(), st.size()) != 0) {
        fprintf(stderr, "a call without room moved the state\n");
        return 1;
    }
    std::vector<mfm_runbatch_event> events(ne);
    if (rc == MFM_E_NOMEM) {
        rc = mfm_hosttwin_runbatch_call(&cfg, state.data(), runs.data(), bits.data(), sev.data(), totals, events.data(), ne, &ne, &flags);
    }
    if (rc != MFM_OK || ne != events.size()) {
        fprintf(stderr, "the second call: %d (%s)\n", rc, g_error);
        return 1;
    }
    if (mfm_hosttwin_runbatch_state_check(cfg.nr_channels, state.data()) != MFM_OK) {
        fprintf(stderr, "the state the call left: %s\n", g_error);
        return 1;
    }
    FILE *f = fopen(argv[3], "wb");
    const uint64_t count = ne;
    bool ok = f && fwrite(&count, 8, 1, f) == 1 && (!ne || fwrite(events.data(), sizeof(mfm_runbatch_event), ne, f) == ne);
    ok = f && fclose(f) == 0 && ok;
    f = fopen(argv[2], "wb");
    ok = f && fwrite(state.data(), 1, st.size(), f) == st.size() && ok;
    ok = f && fclose(f) == 0 && ok;
    printf("{\"events\": %zu}\n", ne);
    return ok ? 0 : 1;
}
