// Stand-alone walk of the host layer's lifecycle for a sanitizer build (`make asan`): the three
// clean scripts of tests/test_hostsim_lifecycle.py and every failed allocation of their grow call.
// TEST INFRASTRUCTURE ONLY; not run by pytest.  The ROM is its own: a ROM-only cartridge that loops
// at its entry point.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "../../include/pokegym_amd.h"

extern "C" int64_t pk_sim_alloc_live(void);
extern "C" int64_t pk_sim_alloc_calls(void);
extern "C" void pk_sim_alloc_fail_at(int64_t k);

namespace {

constexpr uint32_t N = 64, MAX_STEPS = 100, SLOTS = 4, GROW_TO = 800;

struct Ctx {
    bool reward;
    pk_handle* h = nullptr;
    std::vector<uint8_t> rom = std::vector<uint8_t>(0x8000, 0);
    std::vector<uint8_t> acts = std::vector<uint8_t>(N), term = std::vector<uint8_t>(N), trunc = std::vector<uint8_t>(N);
    std::vector<double> rew = std::vector<double>(N);
    uint32_t t = 0;
    explicit Ctx(bool r) : reward(r) { rom[0x100] = 0x18; rom[0x101] = 0xFE; }   // JR -2
};

int step(Ctx& c) {
    for (uint32_t e = 0; e < N; e++) c.acts[e] = (uint8_t)((e * 5 + c.t * 3) % 8);
    c.t++;
    return pk_step(c.h, c.acts.data(), nullptr, c.rew.data(), c.term.data(), c.trunc.data(), nullptr);
}

int create(Ctx& c) {
    pk_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.n_envs = N;
    cfg.rom = c.rom.data();
    cfg.rom_len = c.rom.size();
    cfg.frame_skip = 2;
    cfg.release_frame = 1;
    cfg.flags = PK_F_RENDER | (c.reward ? PK_F_REWARD : 0u);
    cfg.max_episode_steps = MAX_STEPS;
    cfg.reward_scale = 4.0;
    return pk_create(&cfg, &c.h);
}

int steps(Ctx& c) {
    std::vector<int32_t> save(N, -1), load(N, -1);
    save[3] = 0; save[20] = 1; load[9] = 0; load[21] = 1;
    int rc = step(c);
    if (!rc) rc = pk_bank_checkpoint(c.h, save.data(), 0, 32, nullptr);
    if (!rc) rc = step(c);
    if (!rc) rc = pk_bank_resume(c.h, load.data(), 0, 32, nullptr);
    if (!rc) rc = step(c);
    return rc;
}

int probes(Ctx& c) {
    pk_probe p[2];
    memset(p, 0, sizeof p);
    p[0].addr = 0xD361; p[0].op = PK_PO_DELTA;
    p[1].addr = 0xFF80; p[1].op = PK_PO_CHANGE;
    for (pk_probe& q : p) { q.len = 1; q.count = 1; q.weight = 1.0; }
    return pk_probe_create(c.h, p, 2);
}

struct Call { const char* name; std::function<int(Ctx&)> run; };

const Call CREATE{"create", create}, BANK{"bank", [](Ctx& c) { return pk_bank_create(c.h, SLOTS); }},
    TRAJ{"traj", [](Ctx& c) { return pk_traj_enable(c.h); }},
    EPISODES{"episodes", [](Ctx& c) { return pk_bank_enable_episodes(c.h); }},
    GENERIC{"generic", [](Ctx& c) { return pk_bank_enable_generic_episodes(c.h, PK_GEP_PROBES | PK_GEP_STACK); }},
    ARCHIVE{"archive", [](Ctx& c) { return pk_archive_create(c.h, 1, SLOTS - 1, 7); }},
    EXCHANGE{"exchange", [](Ctx& c) { return pk_archive_exchange_enable(c.h); }},
    COUNTS{"counts", [](Ctx& c) { return pk_counts_create(c.h, 10); }},
    FSTACK{"fstack", [](Ctx& c) { return pk_fstack_create(c.h, 4, 2, PK_FSTACK_CHW, PK_FSTACK_MEAN); }},
    PROBES{"probes", probes}, FIRST{"first_steps", step},
    GROW{"grow", [](Ctx& c) { return pk_set_episode_params(c.h, GROW_TO, 4.0); }}, STEPS{"steps", steps},
    DESTROY{"destroy", [](Ctx& c) { pk_destroy(c.h); c.h = nullptr; return 0; }};

struct Script { const char* name; bool reward; std::vector<Call> calls; };

int failures = 0;

void expect(bool ok, const std::string& what) {
    if (ok) return;
    failures++;
    fprintf(stderr, "FAILED: %s (%s)\n", what.c_str(), pk_last_error());
}

// the script with the k-th allocation of its grow call failing first (k < 0: a clean walk);
// returns the allocations of a clean grow
int64_t walk(const Script& s, int64_t k) {
    Ctx c(s.reward);
    const int64_t baseline = pk_sim_alloc_live();
    int64_t grow_allocs = 0;
    for (const Call& call : s.calls) {
        const std::string at = std::string(s.name) + "/" + call.name + " k=" + std::to_string(k);
        if (k >= 0 && !strcmp(call.name, "grow")) {
            const int64_t live = pk_sim_alloc_live();
            pk_sim_alloc_fail_at(k);
            const int rc = call.run(c);
            pk_sim_alloc_fail_at(-1);
            expect(rc < 0 && pk_last_error()[0], at + ": the armed call fails with a message");
            expect(pk_sim_alloc_live() == live, at + ": nothing more is live after the failure");
            expect(step(c) == 0, at + ": a step after the failure");
        }
        const int64_t before = pk_sim_alloc_calls();
        expect(call.run(c) == 0, at);
        if (!strcmp(call.name, "grow")) grow_allocs = pk_sim_alloc_calls() - before;
    }
    expect(pk_sim_alloc_live() == baseline, std::string(s.name) + ": nothing is live after pk_destroy");
    return grow_allocs;
}

}  // namespace

int main() {
    const Script scripts[] = {
        {"reward", true, {CREATE, BANK, TRAJ, EPISODES, ARCHIVE, EXCHANGE, COUNTS, FSTACK, FIRST, GROW, STEPS, DESTROY}},
        {"reward_episodes_first", true, {CREATE, BANK, EPISODES, TRAJ, ARCHIVE, EXCHANGE, COUNTS, FSTACK, FIRST, GROW, STEPS, DESTROY}},
        {"generic", false, {CREATE, PROBES, FSTACK, BANK, TRAJ, GENERIC, ARCHIVE, COUNTS, FIRST, GROW, STEPS, DESTROY}},
    };
    for (const Script& s : scripts) {
        const int64_t n = walk(s, -1);
        expect(n > 0, std::string(s.name) + ": the grow allocates");
        for (int64_t k = 0; k < n; k++) walk(s, k);
        printf("%s: clean walk and %lld failed grows\n", s.name, (long long)n);
    }
    printf(failures ? "%d checks failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
