// compiles and links the long-insertion wrappers of include/s2k.hpp (tests/test_pileup_long.py); run without a GPU it only reports that
// there is none
#include <cstdio>

#include "s2k.hpp"

static_assert(S2K_LONG_INS_MIN == 2 && S2K_LONG_INS_MAX == 12 && S2K_LONG_INS_POS_BITS == 36, "the key layout of include/s2k.h");

int main() {
    std::printf("S2K_LONG_INS_MIN %u\nS2K_LONG_INS_MAX %u\nS2K_LONG_INS_POS_BITS %d\n", S2K_LONG_INS_MIN, S2K_LONG_INS_MAX, S2K_LONG_INS_POS_BITS);
    try {
        s2k::Engine eng(0);
        s2k_walk_out walks{};
        s2k_align_out al{};
        s2k_pile pile{};
        const uint64_t off = 0;
        al.ops_off = const_cast<uint64_t *>(&off);
        const s2k::Engine::Pool pool{nullptr, 0, nullptr, nullptr};
        uint64_t cand = 0;
        const s2k::Engine::PileupKeys k = eng.walks_pileup_ex(walks, nullptr, 0, &off, nullptr, 0, nullptr, 0, pool, al, pile, nullptr, 0, S2K_PILEUP_MAX_SHIFT, &cand);
        const s2k::Engine::Consensus c = eng.pileup_consensus_ex(pile, &off, nullptr, 0, nullptr, 0, 3, nullptr, nullptr, 0);
        std::printf("%llu %llu %llu %llu\n", (unsigned long long)k.stats.v[0], (unsigned long long)k.n_candidates, (unsigned long long)k.n_long_keys,
                    (unsigned long long)c.stats[5]);
    } catch (const s2k::Error &e) {
        std::printf("no engine: %s\n", e.what());
    }
    return 0;
}
