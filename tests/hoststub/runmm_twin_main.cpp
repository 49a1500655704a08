/*
 * runmm_twin_main.cpp - the host code of the burst Mueller-Muller stage (csrc/mfm_runmm.hip: the geometry, the run checks, the
 * host twin) under AddressSanitizer and UBSan, as a program of its own: tests/test_runmm.py builds it together with
 * mfm_runmm.hip with -fsanitize=address,undefined on the host side and runs it on a burst resampler's call it wrote to a file.
 * Every buffer the twin reads or writes is a heap block of exactly the size the call needs, so a step past either end is
 * reported.  No device is looked for: the twin needs none.
 *
 *   runmm_twin IN STATE OUT
 *   IN    uint32 nr_channels, nr_runs, nr_elems, max_decisions; float kw, km, samples_per_bit, error_min, error_max;
 *         nr_runs struct mfm_runrs_run; nr_elems int16
 *   STATE nr_channels struct mfm_runmm_state, read and written back
 *   OUT   uint64 nr_runs, nr_decisions; the run records; the decisions
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
    std::vector<unsigned char> in, st;
    if (!read_file(argv[1], in) || !read_file(argv[2], st) || in.size() < 36) {
        fprintf(stderr, "cannot read the input\n");
        return 2;
    }
    uint32_t head[4];
    float par[5];
    memcpy(head, in.data(), 16);
    memcpy(par, in.data() + 16, 20);
    const size_t nr_runs = head[1], nr_elems = head[2];
    if (in.size() != 36 + nr_runs * sizeof(mfm_runrs_run) + nr_elems * 2 || st.size() != head[0] * sizeof(mfm_runmm_state)) {
        fprintf(stderr, "the input's sizes do not add up\n");
        return 2;
    }
    std::vector<mfm_runrs_run> runs(nr_runs);
    std::vector<int16_t> payload(nr_elems);
    std::vector<mfm_runmm_state> state(head[0]);
    if (nr_runs) {
        memcpy(runs.data(), in.data() + 36, nr_runs * sizeof(mfm_runrs_run));
    }
    if (nr_elems) {
        memcpy(payload.data(), in.data() + 36 + nr_runs * sizeof(mfm_runrs_run), nr_elems * 2);
    }
    memcpy(state.data(), st.data(), st.size());
    mfm_runmm_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.abi_version = MFM_ABI_VERSION;
    cfg.nr_channels = head[0];
    cfg.max_runs = nr_runs ? (uint32_t)nr_runs : 1u;
    cfg.max_out_samples = nr_elems ? (uint32_t)nr_elems : 1u;
    cfg.max_decisions = head[3];
    cfg.kw = par[0];
    cfg.km = par[1];
    cfg.samples_per_bit = par[2];
    cfg.error_min = par[3];
    cfg.error_max = par[4];
    const uint64_t totals[4] = { nr_runs, nr_elems, 0, 0 };
    if (mfm_hosttwin_runmm_state_check(cfg.nr_channels, state.data()) != MFM_OK) {
        fprintf(stderr, "state: %s\n", g_error);
        return 1;
    }
    /* once without room: the sizes needed, and nothing written */
    size_t nr = 0, nd = 0;
    uint32_t flags = 0;
    const std::vector<mfm_runmm_state> before(state);
    int rc = mfm_hosttwin_runmm_call(&cfg, state.data(), runs.data(), payload.data(), totals, nullptr, 0, &nr, nullptr, 0, &nd, &flags);
    if (rc != MFM_OK && rc != MFM_E_NOMEM) {
        fprintf(stderr, "refused (%d, flags %u): %s\n", rc, flags, g_error);
        return 1;
    }
    if (rc == MFM_E_NOMEM && memcmp(before.data(), state.data(), st.size()) != 0) {
        fprintf(stderr, "a call without room moved the state\n");
        return 1;
    }
    std::vector<mfm_runmm_run> out_runs(nr);
    std::vector<int16_t> decisions(nd);
    rc = mfm_hosttwin_runmm_call(&cfg, state.data(), runs.data(), payload.data(), totals, out_runs.data(), nr, &nr, decisions.data(), nd, &nd,
                                 &flags);
    if (rc != MFM_OK || nr != out_runs.size() || nd != decisions.size()) {
        fprintf(stderr, "the second call: %d (%s)\n", rc, g_error);
        return 1;
    }
    if (mfm_hosttwin_runmm_state_check(cfg.nr_channels, state.data()) != MFM_OK) {
        fprintf(stderr, "the state the call left: %s\n", g_error);
        return 1;
    }
    FILE *f = fopen(argv[3], "wb");
    const uint64_t counts[2] = { nr, nd };
    bool ok = f && fwrite(counts, 8, 2, f) == 2 && (!nr || fwrite(out_runs.data(), sizeof(mfm_runmm_run), nr, f) == nr) &&
              (!nd || fwrite(decisions.data(), 2, nd, f) == nd);
    ok = f && fclose(f) == 0 && ok;
    f = fopen(argv[2], "wb");
    ok = f && fwrite(state.data(), 1, st.size(), f) == st.size() && ok;
    ok = f && fclose(f) == 0 && ok;
    printf("{\"runs\": %zu, \"decisions\": %zu}\n", nr, nd);
    return ok ? 0 : 1;
}
