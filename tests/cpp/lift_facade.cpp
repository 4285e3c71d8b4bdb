// compiles and links the lift wrappers of include/s2k.hpp (tests/test_lift.py); run without a GPU it only reports that there is none
#include <cstdio>

#include "s2k.hpp"

int main() {
    try {
        s2k::Engine eng(0);
        s2k_unitig_out outer{};
        eng.unitig_copy_places(outer, 0, nullptr, nullptr, nullptr, 0, nullptr);
        s2k_thread_out paths{}, out{};
        const s2k::Engine::LiftGraph g{};
        const s2k::Engine::LiftTotals t = eng.paths_lift(0, paths, 0, g, out);
        std::printf("%llu %llu %llu %llu\n", (unsigned long long)t.steps, (unsigned long long)t.merged, (unsigned long long)t.dropped,
                    (unsigned long long)t.conflicts);
    } catch (const s2k::Error &e) {
        std::printf("no engine: %s\n", e.what());
    }
    return 0;
}
