// Stand-alone run of injected machine states (tests/state_cases.py) through the host-simulation
// build of K1 for a sanitizer build (`make states_asan`): a program of its own, started as a child
// process by tests/test_hostsim_states.py, never a library loaded into python.  K1 forms LDS and
// image indices from an arbitrary PC, SP, HL and DE (the loop fast paths' `li + 4`, the HRAM mirror
// rows, the fetch paths, the block copies); address and undefined-behaviour sanitizers see an index
// that leaves its array where a GPU run reads garbage silently.  TEST INFRASTRUCTURE ONLY.
//
// Case file: u32 rom_len, n, frame_skip, release_frame, steps; the ROM; n v9 states.
// Prints the states' FNV-1a hash after the last step; any failure is a non-zero exit.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/pokegym_amd.h"

static const size_t V9 = 142610;

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t hd[5];
    if (fread(hd, 4, 5, f) != 5) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t rom_len = hd[0], n = hd[1], steps = hd[4];
    std::vector<uint8_t> rom(rom_len), states((size_t)n * V9), acts(n, 8), out((size_t)n * V9);
    if (fread(rom.data(), 1, rom_len, f) != rom_len || fread(states.data(), 1, states.size(), f) != states.size()) {
        fprintf(stderr, "short case file\n");
        return 2;
    }
    fclose(f);
    pk_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.n_envs = n;
    cfg.rom = rom.data();
    cfg.rom_len = rom_len;
    cfg.frame_skip = hd[2];
    cfg.release_frame = hd[3];
    cfg.flags = PK_F_RENDER;
    cfg.max_episode_steps = 20480;
    cfg.reward_scale = 4.0;
    pk_handle* h = nullptr;
    int rc = pk_create(&cfg, &h);
    for (uint32_t e = 0; e < n && !rc; e++) rc = pk_load_env(h, e, &states[(size_t)e * V9], V9);
    for (uint32_t t = 0; t < steps && !rc; t++) rc = pk_step(h, acts.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
    if (!rc) rc = pk_snapshot_range(h, 0, n, out.data(), out.size());
    if (rc) { fprintf(stderr, "failed (%d): %s\n", rc, pk_last_error()); return 1; }
    pk_destroy(h);
    uint64_t hash = 1469598103934665603ull;
    for (uint8_t b : out) hash = (hash ^ b) * 1099511628211ull;
    printf("%u envs, %u steps: %016llx\n", n, steps, (unsigned long long)hash);
    return 0;
}
