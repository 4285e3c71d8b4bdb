// compiles and links the alignment wrappers of include/s2k.hpp (tests/test_align.py); run without a GPU it only reports that there is none
#include <cstdio>

#include "s2k.hpp"

int main() {
    try {
        s2k::Engine eng(0);
        s2k_walk_out walks{};
        s2k_align_out out{};
        const uint64_t off = 0;
        const uint64_t n = eng.walks_targets(walks, nullptr, 0, &off, nullptr, 0, nullptr, 0);
        const s2k::Engine::Pool pool{nullptr, 0, nullptr, nullptr};
        const uint64_t m = eng.align_pairs(pool, pool, 0, S2K_ALIGN_MAX_EDITS, &out);
        std::printf("%llu %llu\n", (unsigned long long)n, (unsigned long long)m);
    } catch (const s2k::Error &e) {
        std::printf("no engine: %s\n", e.what());
    }
    return 0;
}
