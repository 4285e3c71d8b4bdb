// compiles and links the pile-up wrappers of include/s2k.hpp (tests/test_pileup.py); run without a GPU it only reports that there is none
#include <cstdio>

#include "s2k.hpp"

int main() {
    try {
        s2k::Engine eng(0);
        s2k_walk_out walks{};
        s2k_align_out al{};
        s2k_pile pile{};
        const uint64_t off = 0;
        al.ops_off = const_cast<uint64_t *>(&off);
        const s2k::Engine::Pool pool{nullptr, 0, nullptr, nullptr};
        const s2k::Engine::PileupStats st = eng.walks_pileup(walks, nullptr, 0, &off, nullptr, 0, nullptr, 0, pool, al, pile);
        const s2k::Engine::Consensus c = eng.pileup_consensus(pile, &off, nullptr, 0, nullptr, 0, 3);
        std::printf("%llu %llu\n", (unsigned long long)st.v[0], (unsigned long long)c.n_new_bases);
    } catch (const s2k::Error &e) {
        std::printf("no engine: %s\n", e.what());
    }
    return 0;
}
