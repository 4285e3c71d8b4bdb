// compiles and links the GAF wrapper of include/s2k.hpp (tests/test_gaf_device.py); run without a GPU it only reports that there is
// none
#include <cstdio>

#include "s2k.hpp"

int main() {
    try {
        s2k::Engine eng(0);
        const uint64_t off[2] = {0, 0};
        s2k_walk_out walks{};
        walks.walk_off = const_cast<uint64_t *>(off);
        s2k_align_out al{};
        al.flags = const_cast<uint32_t *>(reinterpret_cast<const uint32_t *>(off));
        al.ops_off = const_cast<uint64_t *>(off);
        const uint64_t plain = eng.walks_gaf(0, walks, 0, nullptr, 0);
        const uint64_t aligned = eng.walks_gaf(0, walks, 0, nullptr, 0, s2k::Engine::Names{nullptr, nullptr, 0}, 1000000000000ull, nullptr, &al, nullptr, 0, nullptr);
        std::printf("%llu %llu\n", (unsigned long long)plain, (unsigned long long)aligned);
    } catch (const s2k::Error &e) {
        std::printf("no engine: %s\n", e.what());
    }
    return 0;
}
